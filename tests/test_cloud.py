"""Point clouds, CPU side: the numpy restatement of Utility::dmap2pcl's loop and
ply::write's grey (tests/cloud_restate.py) pins what the kernels are compared with
bit for bit in tests/test_gpu_cloud.py, the library declares and exports the new
entry points, and the new kernels carry no scratch.

The ladders: z depends on the disparity value alone (about 576 414 mm / v with
tests/golden/q_matrix.json), z - mn is exact in float32 for these magnitudes, so
the pinned grey and its near misses part only where the float32 quotient, times
255, falls on the other side of an integer than the double one -- a few pixels
per map at most, and none on most value ranges.  The ranges below were found by
scanning lo 1..39, hi up to lo + 3000 for ranges on which both near misses show.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests import cloud_restate as ref
from tests.conftest import GOLDEN
from tests.test_kernel_scratch import LIB, LLVM, kernel_scratch

Q_REF = np.array(json.load(open(os.path.join(GOLDEN, "q_matrix.json")))["Q"], np.float32)
LADDERS = [(2, 9), (36, 362), (39, 938), (37, 2056)]
LADDER_SHAPE = (70, 100)

NEW_SYMBOLS = ["mvsv_point_cloud_device", "mvsv_point_cloud", "mvsv_stream_enable_cloud", "mvsv_stream_disable_cloud",
               "mvsv_stream_front_cloud", "mvsv_stream_front_cloud_device"]


def test_library_exports_the_cloud_entry_points():
    from mvstereovision3_amd import _lib
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name
    import mvstereovision3_amd as mvsv
    assert callable(mvsv.point_cloud) and mvsv.CLOUD_DTYPE == ref.CLOUD_DTYPE and mvsv.CLOUD_DTYPE.itemsize == 16
    assert "point_cloud" in mvsv.__all__ and "CLOUD_DTYPE" in mvsv.__all__
    for m in ("enable_cloud", "disable_cloud", "front_cloud"):
        assert callable(getattr(mvsv.DisparityStream, m))
    # no device needed: a null handle is refused before anything else
    E = _lib.MVSV_E_INVALID_ARG
    assert lib.mvsv_point_cloud_device(None, 1, None, 0, 0, 0, 0, None, None, 0, None, None) == E
    assert lib.mvsv_point_cloud(None, None, 0, 0, 0, None, None, 0, None, None) == E
    assert lib.mvsv_stream_enable_cloud(None, None, None, 0) == E
    assert lib.mvsv_stream_disable_cloud(None) == E
    assert lib.mvsv_stream_front_cloud(None, None, 0, None, None) == E
    assert lib.mvsv_stream_front_cloud_device(None, None, None, None) == E


def test_fixed_cases(oracle, mvsv):
    assert callable(mvsv.point_cloud)
    # the arithmetic of the grey on hand-made numbers
    assert ref.grey([10.0, 4.0, 7.0, 3.0], 4, 10).tolist() == [255, 0, 127, -42]  # 127.5 and -42.5 truncate
    assert ref.grey([1000.0], 1, 2).tolist() == [254745]  # not clamped to 0..255
    assert ref.grey([5.0, 7.0, 3.0], 5, 5).tolist() == [ref.INT32_MIN] * 3  # 0 / 0, +inf, -inf
    assert ref.grey([3e9], 1, 2).tolist() == [ref.INT32_MIN]  # beyond int32
    assert ref.grey([8421505.0], 0, 1).tolist() == [ref.INT32_MIN]  # 2 147 483 775 is one step too far
    assert ref.grey([-8421504.0], 0, 1).tolist() == [-2147483520]  # the last products int32 still holds
    assert ref.grey([8421504.0], 0, 1).tolist() == [2147483520]
    assert ref.minmax(np.array([[0, -16, 7, 3]], np.int16)) == (3, 7)
    assert ref.minmax(np.array([[0, -16]], np.int16)) == (32767, -32768)
    # order and coordinates: raster order, the oracle's points, invalid pixels dropped
    d = np.array([[0, 16, -16], [32, 0, 48]], np.int16)
    rec, mm = ref.cloud(d, Q_REF, oracle.reproject)
    assert mm == (16, 48) and len(rec) == 3
    pts = oracle.reproject(d, Q_REF)
    for k, (r, c) in enumerate([(0, 1), (1, 0), (1, 2)]):
        assert rec[["x", "y", "z"]][k].tolist() == tuple(pts[r, c, :3].tolist())
        x, y, z, _ = mvsv.Utility.calcCoordinate(mvsv.dMapValues(float(d[r, c]), c, r), Q_REF)
        assert (rec["x"][k], rec["y"][k], rec["z"][k]) == (x, y, z)
    assert rec["grey"].tolist() == ref.grey(rec["z"], 16, 48).tolist()
    none, mm = ref.cloud(np.array([[0, -16]], np.int16), Q_REF, oracle.reproject)
    assert len(none) == 0 and mm == (32767, -32768)
    const, mm = ref.cloud(np.full((3, 5), 77, np.int16), Q_REF, oracle.reproject)
    assert mm == (77, 77) and len(const) == 15 and (const["grey"] == ref.INT32_MIN).all()


@pytest.mark.parametrize("lo,hi", LADDERS)
def test_ladders_tell_the_pinned_grey_from_its_near_misses(oracle, mvsv, lo, hi):
    """A kernel that computes the grey wholly in double, or multiplies by the
    reciprocal of the range, differs from the restatement on each of these
    ladders; every grey stays inside int32."""
    assert callable(mvsv.point_cloud)
    d = ref.ladder(lo, hi, LADDER_SHAPE)
    want, mm = ref.cloud(d, Q_REF, oracle.reproject)
    assert mm == (lo, hi) and len(want) == hi - lo + 1
    assert (np.diff(want["z"]) < 0).all()  # the ladder's order survives: z falls as v rises
    n64 = int((want["grey"] != ref.cloud(d, Q_REF, oracle.reproject, ref.grey_f64)[0]["grey"]).sum())
    nrc = int((want["grey"] != ref.cloud(d, Q_REF, oracle.reproject, ref.grey_recip)[0]["grey"]).sum())
    print(f"ladder ({lo}, {hi}): {n64} greys differ from float64, {nrc} from a reciprocal multiply")
    assert n64 >= 1 and nrc >= 1
    t = (want["z"].astype(np.float64) - lo) / (hi - lo) * 255.0
    assert (np.abs(t) < 2.0 ** 31 - 1).all() and (want["grey"] != ref.INT32_MIN).all()


def test_random_maps_keep_every_grey_inside_int32(oracle):
    for seed, shape in [(1, (480, 640)), (2, (70, 100)), (3, (4099, 3))]:
        rec, (mn, mx) = ref.cloud(ref.random_map(seed, shape), Q_REF, oracle.reproject)
        assert mn < mx and (rec["grey"] != ref.INT32_MIN).all()


def test_ply_writer_prints_the_restated_greys(oracle, mvsv, tmp_path):
    """mvsv_write_ply's WITH_COLOR grey is the record's grey, INT32_MIN case included."""
    for name, d in [("ladder", ref.ladder(2, 9, LADDER_SHAPE)), ("random", ref.random_map(7, (33, 41))),
                    ("const", np.full((2, 3), 500, np.int16))]:
        rec, _ = ref.cloud(d, Q_REF, oracle.reproject)
        path = str(tmp_path / f"{name}.ply")
        xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=1)
        assert mvsv.ply("a", "b", d).write(path, xyz, mvsv.ply.WITH_COLOR)
        lines = open(path).read().split("end_header\n")[1].splitlines()
        assert len(lines) == len(rec)
        greys = [[int(t) for t in ln.split()[3:]] for ln in lines]
        assert greys == [[g, g, g] for g in rec["grey"].tolist()], name


def test_header_lists_the_reference_counterparts():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mvsv.h")).read()
    table = text[:text.index("#ifndef")] if "#ifndef" in text else text
    for name in ("mvsv_point_cloud", "mvsv_stream_enable_cloud", "_front_cloud"):
        assert name in table, f"{name} missing from the header's table of reference counterparts"
    for name in NEW_SYMBOLS:
        assert re.search(rf"MVSV_API int {name}\(", text), name


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"),
                    reason="library not built / no ROCm llvm tools")
def test_cloud_kernels_have_no_scratch():
    ks = kernel_scratch()
    for pat in (r"cloud_rows_kernel", r"cloud_scan_kernel", r"cloud_scatter_kernel"):
        picked = {k: v for k, v in ks.items() if re.search(pat, k)}
        assert picked, f"no kernel matches {pat}"
        assert not any(picked.values()), f"kernels with scratch: {picked}"
