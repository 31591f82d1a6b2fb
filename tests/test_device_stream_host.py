"""Host side of the stream's device ends (no GPU): ring_push_segments and the
pointer classification of mvsv_ring.hpp in a stand-alone program under ASan + UBSan,
and the declarations of the new entry points in include/mvsv.h, _lib.py and the
package."""
import ctypes
import os
import re
import subprocess

from tests.conftest import ROOT

P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
PP = ctypes.POINTER(P)
PUSH = [P, I, P, Z, Z, P, Z, Z, P]
NEW_FUNCTIONS = {
    "mvsv_stream_push_device": PUSH,
    "mvsv_stream_push_raw_device": PUSH,
    "mvsv_stream_push_bgr_device": PUSH,
    "mvsv_stream_set_host_outputs": [P, I],
    "mvsv_stream_pop_device": [P, P, Z, P, P],
    "mvsv_stream_front_map_device": [P, PP, P],
    "mvsv_stream_front_rectified_device": [P, PP, PP],
    "mvsv_stream_front_display_device": [P, PP, P],
    "mvsv_stream_front_view_device": [P, PP, P],
    "mvsv_stream_fence": [P, P],
}
HOST_BITS = {"MVSV_HOST_MAP": 1, "MVSV_HOST_RECTIFIED": 2, "MVSV_HOST_DISPLAY": 4, "MVSV_HOST_VIEW": 8,
             "MVSV_HOST_ALL": 15}


def test_ring_segments_and_pointer_classes_under_asan_ubsan(tmp_path):
    exe = tmp_path / "ring_segments_check"
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "mvstereovision3_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "ring_segments_check.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ)
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout and "segments:" in r.stdout and "sources:" in r.stdout
    assert "slot blocks:" in r.stdout and "push geometry:" in r.stdout


def c_params(decl):
    """ctypes classes of a C parameter list of include/mvsv.h."""
    out = []
    for p in decl.split(","):
        p = " ".join(p.split())
        if p.count("*") == 2:
            out.append(PP)
        elif "*" in p:
            out.append(P)
        elif p.startswith("size_t"):
            out.append(Z)
        else:
            assert p.startswith("int "), p
            out.append(I)
    return out


def test_header_and_binding_declare_the_device_ends(mvsv):
    from mvstereovision3_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvsv.h")).read()
    lib = _lib.lib()
    for name, want in NEW_FUNCTIONS.items():
        m = re.search(r"MVSV_API\s+int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in mvsv.h"
        assert c_params(m.group(1)) == want, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want, name
    for name, value in HOST_BITS.items():
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", hdr)
        assert m and int(m.group(1)) == value, name
        assert getattr(_lib, name) == value and getattr(mvsv, name) == value and name in mvsv.__all__, name
    for method in ("host_outputs", "fence", "front_map", "front_rectified"):
        assert hasattr(mvsv.DisparityStream, method), method


def test_cpp_mirror_declares_the_device_ends():
    for header, names in (("mvsv_detection.hpp", ("pushDevice", "pushBgrDevice", "popDevice", "frontMapDevice",
                                                   "hostOutputs", "fence")),
                          ("mvsv_stereosystem.hpp", ("pushDevice", "popDevice", "frontMapDevice", "hostOutputs",
                                                     "fence"))):
        text = open(os.path.join(ROOT, "include", header)).read()
        for n in names:
            assert re.search(r"\b" + n + r"\s*\(", text), f"{header}: {n}"
