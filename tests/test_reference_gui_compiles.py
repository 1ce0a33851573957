"""The reference's own src/RendererGUI.cpp -- the one caller of RendererCore (a friend that reads and writes its private
fields, include/RendererCore.h:18) -- goes through a compiler against integration/RendererCoreShim.h, UNCHANGED and where it
lies: build container only (skipped where /root/reference is absent; nothing of the reference is copied or committed).

How the substitution works without touching the reference tree: RendererGUI.h includes "RendererCore.h" with quotes, which
finds the reference's header next to it; the shim is therefore pre-included (-include) and owns the same include guard
(RENDERERCORE_H), so the reference's header is read as empty.  glad / GLFW / glm are not vendored by the reference and not
installed here: integration/stub/ holds stand-in declarations of the handful of names RendererGUI.cpp, GlfwManager.h and the
widget headers use -- syntax only, nothing is linked.  Dear ImGui, the file browser and the transfer-function widget headers
are the reference's own (vendored).

-fpermissive: src/RendererGUI.cpp:42 takes the address of a bound member function (`&(volren.main_cam.setOrientation)`),
which ISO C++ forbids -- against the reference's own Camera class just as against the shim's; GCC accepts it under
-fpermissive and binds it to `&CameraProxy::setOrientation`, which is what the shim expects.
"""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")


@pytest.mark.skipif(not os.access(REF / "src" / "RendererGUI.cpp", os.R_OK), reason="the reference tree is only present in the build container")
@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_reference_renderergui_compiles_against_the_shim(std):
    cmd = ["g++", f"-std={std}", "-fsyntax-only", "-fpermissive", "-include", "glad/glad.h", "-include", str(ROOT / "integration" / "RendererCoreShim.h"),
           f"-I{ROOT / 'integration' / 'stub'}", f"-I{ROOT / 'include'}", f"-I{ROOT / 'integration'}",
           f"-I{REF / 'include'}", f"-I{REF / 'include' / 'UI'}", f"-I{REF}", str(REF / "src" / "RendererGUI.cpp")]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    # the one diagnostic is the reference's own non-standard bind, nothing about the shim's members
    errors = [l for l in proc.stderr.splitlines() if "error" in l]
    assert not errors, errors
    warned = [l for l in proc.stderr.splitlines() if "warning:" in l]
    assert all("bound member function" in l for l in warned), warned


@pytest.mark.skipif(not os.access(REF / "src" / "RendererGUI.cpp", os.R_OK), reason="the reference tree is only present in the build container")
def test_without_permissive_only_the_references_own_line_42_fails():
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-include", "glad/glad.h", "-include", str(ROOT / "integration" / "RendererCoreShim.h"),
           f"-I{ROOT / 'integration' / 'stub'}", f"-I{ROOT / 'include'}", f"-I{ROOT / 'integration'}",
           f"-I{REF / 'include'}", f"-I{REF / 'include' / 'UI'}", f"-I{REF}", str(REF / "src" / "RendererGUI.cpp")]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    errors = [l for l in proc.stderr.splitlines() if " error: " in l]
    assert len(errors) == 1 and "RendererGUI.cpp:42:" in errors[0] and "bound member function" in errors[0], proc.stderr
