// vr_code_unit.h -- one line per .hip file that is compiled as a device code object (a "unit"): VR_CODE_UNIT defines the unit's
// empty kernel and registers a launcher for it.  Launching the empty kernel makes the HIP runtime inflate and load that unit's
// code object (a cold first launch costs ~16 ms otherwise); launch_warm_units() does that for every unit of a group.
// The Makefile tells code_units.cpp how many kernel objects it links: a unit without its line is an error, not a slow frame.
#pragma once
#include <hip/hip_runtime.h>

namespace vr {

enum WarmGroup { WARM_LOAD_SHADER = 0,    // everything vr_load_shader pre-loads
                 WARM_TRILINEAR = 1 };    // the vr_tslab.hip units: vr_set_filter(TRILINEAR)

typedef hipError_t (*WarmLauncher)(hipStream_t);

// Appends to a fixed, zero-initialised table (no heap, nothing to construct first); a full table still counts.
struct CodeUnitRegistrar {
    CodeUnitRegistrar(const char *family, WarmGroup group, WarmLauncher launch);
};

// One empty launch per registered unit of `group`, in link order; the first error, with *family naming the unit's family.
// hipErrorInvalidValue and *family = nullptr when the units registered are not the kernel objects linked.
hipError_t launch_warm_units(WarmGroup group, hipStream_t st, const char **family);

}  // namespace vr

#define VR_UNIT_PASTE_(a, b) a##b
#define VR_UNIT_PASTE(a, b) VR_UNIT_PASTE_(a, b)
// inside namespace vr, once per unit: NAME + NUM (a unit number macro, or empty) name the kernel, FAMILY is the error text
#define VR_CODE_UNIT(NAME, NUM, FAMILY, GROUP)                                                                  \
    __global__ void VR_UNIT_PASTE(warm_kernel_##NAME, NUM)() {}                                                 \
    namespace {                                                                                                 \
    hipError_t warm_this_unit(hipStream_t st)                                                                   \
    {                                                                                                           \
        hipLaunchKernelGGL(VR_UNIT_PASTE(warm_kernel_##NAME, NUM), dim3(1), dim3(64), 0, st);                   \
        return hipGetLastError();                                                                               \
    }                                                                                                           \
    const CodeUnitRegistrar this_unit_registrar(FAMILY, GROUP, warm_this_unit);                                 \
    }
