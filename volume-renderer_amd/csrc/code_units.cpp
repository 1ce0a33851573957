// code_units.cpp -- the table behind vr_code_unit.h.  VR_KERNEL_UNITS is the number of kernel objects the Makefile links.
#include "vr_code_unit.h"

#ifndef VR_KERNEL_UNITS
#error "VR_KERNEL_UNITS: the Makefile passes the number of kernel objects it links"
#endif

namespace vr {

namespace {
struct CodeUnit { const char *family; WarmGroup group; WarmLauncher launch; };
constexpr int kMaxUnits = 64;
static_assert(VR_KERNEL_UNITS <= kMaxUnits, "raise kMaxUnits");
CodeUnit g_units[kMaxUnits];    // static storage: zero before any registrar runs
int g_registered;
}  // namespace

CodeUnitRegistrar::CodeUnitRegistrar(const char *family, WarmGroup group, WarmLauncher launch)
{
    if (g_registered < kMaxUnits) g_units[g_registered] = CodeUnit{family, group, launch};
    g_registered++;
}

hipError_t launch_warm_units(WarmGroup group, hipStream_t st, const char **family)
{
    *family = nullptr;
    if (g_registered != VR_KERNEL_UNITS) return hipErrorInvalidValue;
    for (int i = 0; i < g_registered; i++) {
        if (g_units[i].group != group) continue;
        *family = g_units[i].family;
        const hipError_t e = g_units[i].launch(st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace vr
