"""Launches that reach the kernel forms only switches and full frames select (no GPU,
fixed seeds).

The SGBM launch plan (mvsv_sgbm_plan.hpp) and mvsv_create pick the kernel form from the
launch size, the CU count and environment switches; on a 256-CU device a small launch
always lands in the "small launch" cell.  Every case here is a small launch that is
switched into another cell:

1. ``ty``    cost tile heights above 16 rows (MVSV_COST_TY), image heights around them
2. ``xcd``   the XCD band permutation of sgbm_cost2_kernel ((row bands x frames) % 8 == 0),
             with MVSV_COST_XCD unset and 0, and a control it does not apply to
3. ``gen``   the general kernels on shapes the specialised ones also cover (MVSV_KERNELS)
4. ``lines`` where the L->R lines of the packed strips run (MVSV_LINES_AUX 0 / 1 / 2);
             two different batches A, B, A back to back on one context

A case names the environment of a fresh context (``env``), the same choice as
KernelOptions fields (``opts``; both are written from one list of switches, see
``_switches``), the matcher parameters, the launch (``n`` frames of ``W`` x ``H``), the
input recipe and the form it is meant to reach, as plan fields (``form``).
tests/test_kernel_forms.py checks on the CPU that the plan of every case has the stated
form at 256 CUs; tests/test_gpu_kernel_forms.py runs the cases on the device.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

CUS = 256  # the CU count the forms are stated for (MI355X)

# kind: "sgbm" (grey), "bgr" (colour entry point, one live channel), "bm"
# recipe: "rand_pair" (tests.test_gpu_parity.rand_pair) or "synth_pair" (mvsv.synth_pair)
Case = namedtuple("Case", "name group kind env opts params n W H recipe seed form")

# SgbmFamily / SgbmAcc of mvsv_sgbm_plan.hpp
GENERIC, PACKED16, PACKED8, BITSLICE = 0, 1, 2, 3
NIB, U8, U16, WORDS = 4, 8, 16, 32

# KernelOptions defaults, in the column order of tests/cpp/kernel_forms_check.cpp
OPTION_FIELDS = ("cost2", "path16", "tri", "cost_fixed_pp", "cost_ty", "path_sched", "lines_aux", "cost_xcd", "bitslice")
OPTION_DEFAULTS = dict(cost2=1, path16=1, tri=1, cost_fixed_pp=1, cost_ty=0, path_sched=0, lines_aux=-1, cost_xcd=1,
                       bitslice=1, bm2=1)
# the columns it prints
PLAN_FIELDS = ("family", "sched", "cost2", "cost_ty", "residual", "acc", "nplanes", "split", "nw", "lpc", "waves",
               "lines_aux", "bits", "stg", "ppc", "gx", "gyn")

# mvsv_create: the words of MVSV_KERNELS and the integer switches
KERNEL_WORDS = {"cost-lds": "cost2", "path-wave": "path16", "path-lines": "tri", "cost-generic": "cost_fixed_pp",
                "bm-tile": "bm2"}
ENV_INTS = {"MVSV_COST_TY": "cost_ty", "MVSV_PATH_SCHEDULE": "path_sched", "MVSV_LINES_AUX": "lines_aux",
            "MVSV_COST_XCD": "cost_xcd"}
# every variable mvsv_create reads for the launch shape: a test clears them all first
ENV_ALL = ("MVSV_KERNELS", "MVSV_COST_TY", "MVSV_PATH_SCHEDULE", "MVSV_STRIP_WAVES", "MVSV_TRI32", "MVSV_FINAL_SPLIT",
           "MVSV_COST_RESIDUAL", "MVSV_BM_TY", "MVSV_STRIP_ORDER", "MVSV_LINES_AUX", "MVSV_BITSLICE", "MVSV_GRAPHS",
           "MVSV_BS_SERIAL", "MVSV_COST_XCD", "MVSV_BS_FUSE", "MVSV_BS_GROUPS", "MVSV_BS_LDSPAD", "MVSV_TRI_STATS",
           "MVSV_TRI_TRACE", "MVSV_BS_STATS", "MVSV_STRIP_SPIN_LIMIT")


def _switches(kernels=(), **ints):
    """(env, opts) of one choice: MVSV_KERNELS words and MVSV_* integers by option field name."""
    env, opts = {}, dict(OPTION_DEFAULTS)
    if kernels:
        env["MVSV_KERNELS"] = ",".join(kernels)
        for w in kernels:
            opts[KERNEL_WORDS[w]] = 0
    names = {v: k for k, v in ENV_INTS.items()}
    for field, v in ints.items():
        env[names[field]] = str(v)
        opts[field] = v
    return env, opts


def sgbm_params(D, bs, P1=0, P2=0, minD=0, disp12=1, cap=0, uniq=10, speckle=(0, 0), mode=0):
    return dict(min_disparity=minD, num_disparities=D, block_size=bs, p1=P1, p2=P2, disp12_max_diff=disp12,
                pre_filter_cap=cap, uniqueness_ratio=uniq, speckle_window_size=speckle[0], speckle_range=speckle[1],
                mode=mode)


def bm_rand_params(rng, bs, D):
    """tests.test_gpu_bm_lanes.rand_params (restated: that module is GPU-marked as a whole)."""
    return dict(pre_filter_type=int(rng.choice([0, 1])), pre_filter_size=int(rng.choice([5, 9])),
                pre_filter_cap=int(rng.integers(1, 64)), block_size=bs,
                min_disparity=int(rng.integers(-8, 8)), num_disparities=D,
                texture_threshold=int(rng.choice([0, 10, 200])),
                uniqueness_ratio=int(rng.choice([0, 5, 15, 60])),
                speckle_window_size=0, speckle_range=0,
                disp12_max_diff=int(rng.choice([-1, 0, 2])))


def plan_bits(form):
    """SgbmPlan::bits() of a stated form (the MVSV_PLAN_* word of mvsv_sgbm_plan)."""
    return ((1 if form["family"] == BITSLICE else 0) | (2 if form["sched"] == 2 else 0) |
            (4 if form["sched"] == 1 else 0) | (8 if form["residual"] else 0))


def xcd_permutes(opts, form):
    """sgbm_cost2_kernel renumbers its blocks: the register-ring kernel, (row bands x frames) % 8 == 0."""
    return bool(form["cost2"] and opts["cost_xcd"] and form["gyn"] % 8 == 0)


TILE_HEIGHTS = (24, 32, 48, 64, 96, 120)


def _heights(TY):
    # a tile taller than the image, a last tile of one row, three tiles with a short last one
    return (TY - 1, TY + 1, 2 * TY + 3)


@lru_cache(maxsize=None)
def all_cases():
    cs = []
    seed = [4000]

    def add(name, group, kind, sw, params, n, W, H, recipe, **form):
        env, opts = sw
        if kind != "bm":
            form.setdefault("split", 0)
            form["bits"] = plan_bits(form)
        seed[0] += 1
        cs.append(Case(name, group, kind, env, opts, params, n, W, H, recipe, seed[0], form))

    # ---- 1. tile heights --------------------------------------------------------------
    # widths D + 70: W1 = 70, two tile columns at D 64 (TX 64), three at D 128 (TX 32), the
    # right one clamped
    for TY in TILE_HEIGHTS:
        for H in _heights(TY):
            gy = -(-H // TY)
            # register-ring kernel + residual plane; mode 1: the pinned bottom rows y >= H - 2
            # in a one-row last tile (H = TY + 1)
            for mode in (0, 1):
                add(f"ty{TY}-H{H}-res-mode{mode}", "ty", "sgbm", _switches(cost_ty=TY),
                    sgbm_params(64, 5, mode=mode, uniq=5 * mode), 1, 134, H, "rand_pair",
                    family=PACKED16, sched=2, cost2=1, cost_ty=TY, residual=1, acc=NIB, nplanes=7 if mode else 4, nw=1,
                    stg=1, ppc=0, gx=2, gyn=gy)
    for TY in (24, 120):
        for i, H in enumerate(_heights(TY)):
            gy = -(-H // TY)
            # blockSize 15 at D 128: five of the window's ring slots in LDS, general P2
            mode = i % 2
            add(f"ty{TY}-H{H}-bs15", "ty", "sgbm", _switches(cost_ty=TY),
                sgbm_params(128, 15, P1=8, P2=32, mode=mode, uniq=10, speckle=(20, 2)), 1, 198, H, "synth_pair",
                family=PACKED16, sched=2, cost2=1, cost_ty=TY, residual=0, acc=U16 if mode else U8,
                nplanes=7 if mode else 4, nw=0, stg=1, ppc=64, gx=3, gyn=gy)
            # the bit-sliced emission (C' planes), both schedules
            for sched in (1, 2):
                add(f"ty{TY}-H{H}-bits-sched{sched}", "ty", "sgbm", _switches(cost_ty=TY, path_sched=sched),
                    sgbm_params(128, 9, P1=2, P2=5, mode=1, uniq=0), 1, 198, H, "rand_pair",
                    family=BITSLICE, sched=sched, cost2=1, cost_ty=TY, residual=0, acc=WORDS,
                    nplanes=4 if sched == 1 else 8, nw=0, waves=9 if sched == 1 else 0, lines_aux=1 if sched == 1 else 0,
                    stg=1, ppc=64, gx=3, gyn=gy)
            # the LDS-ring kernel (blockSize 17), a BGR pair through the colour entry point
            add(f"ty{TY}-H{H}-lds-bgr", "ty", "bgr", _switches(cost_ty=TY),
                sgbm_params(32, 17, mode=1, uniq=10), 1, 102, H, "rand_pair",
                family=PACKED16, sched=2, cost2=0, cost_ty=TY, residual=0, acc=NIB, nplanes=7, nw=0)

    # ---- 2. band permutation ----------------------------------------------------------
    # default tile height 16; bands x frames 8, 8, 24 and the control 9
    for H, n in ((128, 1), (64, 2), (40, 8), (48, 3)):
        gyn = -(-H // 16) * n
        for xcd in (None, 0):
            sw = _switches() if xcd is None else _switches(cost_xcd=0)
            tag = f"H{H}x{n}-{'xcd' if xcd is None else 'noxcd'}"
            # D 128 (TX 32), W1 = 75: three tile columns; packed planes (uniquenessRatio 10)
            add(f"xcd-{tag}-packed", "xcd", "sgbm", sw, sgbm_params(128, 7, mode=1, uniq=10), n, 203, H, "rand_pair",
                family=PACKED16, sched=2, cost2=1, cost_ty=16, residual=1, acc=NIB, nplanes=7, nw=1, stg=1, ppc=64,
                gx=3, gyn=gyn)
            # ... W1 = 62: two tile columns; bit-sliced, MODE_SGBM (copied rows and column 0)
            add(f"xcd-{tag}-bits", "xcd", "sgbm", sw, sgbm_params(128, 13, P1=2, P2=5, mode=0, uniq=0), n, 190, H,
                "synth_pair", family=BITSLICE, sched=2, cost2=1, cost_ty=16, residual=0, acc=WORDS, nplanes=5, nw=0,
                stg=1, ppc=64, gx=2, gyn=gyn)
            # D 32 (TX 128), W1 = 300: three tile columns
            add(f"xcd-{tag}-D32", "xcd", "sgbm", sw, sgbm_params(32, 5, mode=0, uniq=5), n, 332, H, "rand_pair",
                family=PACKED16, sched=2, cost2=1, cost_ty=16, residual=1, acc=NIB, nplanes=4, nw=1, stg=1, ppc=0,
                gx=3, gyn=gyn)

    # ---- 3. general kernels -----------------------------------------------------------
    BYTE, WIDE = (8, 31), (648, 2592)  # 8 * P2 <= 255: byte planes; u16 planes
    # path-wave: sgbm_path_kernel / sgbm_final_kernel, one launch per direction (full forms at D 128 / 256)
    for i, D in enumerate((16, 32, 64, 128, 256)):
        for mode in (0, 1):
            for pen in (BYTE, WIDE):
                uniq = 10 * ((i + mode + (pen is WIDE)) % 2)
                add(f"path-wave-D{D}-mode{mode}-{'u8' if pen is BYTE else 'u16'}", "gen", "sgbm",
                    _switches(("path-wave",)), sgbm_params(D, (3, 5, 7, 9, 11)[i], *pen, mode=mode, uniq=uniq, disp12=1),
                    1, D + 90, 41, "rand_pair",
                    family=GENERIC, sched=0, cost2=1, cost_ty=16, residual=0, acc=U8 if pen is BYTE else U16, nplanes=1,
                    nw=0, stg=2 if D == 16 else 1, ppc={128: 64, 256: 128}.get(D, 0), launches=7 if mode else 4)
    # cost-lds: sgbm_cost_kernel<1> on grey pairs with blockSize <= 15
    for j, D in enumerate((32, 128)):
        for i, bs in enumerate((1, 3, 9, 15)):
            mode = (i + j) % 2
            add(f"cost-lds-D{D}-bs{bs}", "gen", "sgbm", _switches(("cost-lds",)),
                sgbm_params(D, bs, mode=mode, uniq=0 if D == 128 else 10, minD=(-2, 3)[j]), 1, D + 70, 37, "rand_pair",
                family=PACKED16, sched=2, cost2=0, cost_ty=16, residual=0, acc=NIB, nplanes=7 if mode else 4, nw=1)
    # the whole general pipeline
    for D, mode in ((64, 1), (128, 0)):
        add(f"cost-lds-path-wave-D{D}", "gen", "sgbm", _switches(("cost-lds", "path-wave")),
            sgbm_params(D, 7, *BYTE, mode=mode, uniq=10, speckle=(20, 2)), 1, D + 90, 41, "synth_pair",
            family=GENERIC, sched=0, cost2=0, cost_ty=16, residual=0, acc=U8, nplanes=1, nw=0, launches=7 if mode else 4)
    # path-lines: launch_paths_lines16, the 16-lane kernels one launch per direction
    for i, D in enumerate((32, 64, 128, 256)):
        for mode in (0, 1):
            for pen in (BYTE, WIDE):
                add(f"path-lines-D{D}-mode{mode}-{'u8' if pen is BYTE else 'u16'}", "gen", "sgbm",
                    _switches(("path-lines",), path_sched=1),
                    sgbm_params(D, (5, 9, 3, 7)[i], *pen, mode=mode, uniq=10 * ((i + mode) % 2)), 1, D + 90, 41,
                    "rand_pair", family=PACKED16, sched=0, cost2=1, cost_ty=16, residual=0,
                    acc=U8 if pen is BYTE else U16, nplanes=1, nw=0, stg=1, ppc={128: 64, 256: 128}.get(D, 0),
                    launches=7 if mode else 4)
    # cost-generic: sgbm_cost2_kernel<*, *, 0, false> at D 128 / 256
    for j, D in enumerate((128, 256)):
        for i, bs in enumerate((3, 9, 15)):
            mode = (i + j) % 2
            add(f"cost-generic-D{D}-bs{bs}", "gen", "sgbm", _switches(("cost-generic",)),
                sgbm_params(D, bs, P1=2, P2=5, mode=mode, uniq=0), 1, D + 70, 37, "rand_pair",
                family=PACKED16, sched=2, cost2=1, cost_ty=16, residual=1 if D == 128 else 0, acc=NIB,
                nplanes=7 if mode else 4, nw=1, stg=1, ppc=0)
    # bm-tile: bm_match_kernel where the lanes kernel applies (blockSize <= 21, D <= 128)
    for bs in (5, 9, 15, 21):
        for D in (16, 64, 128):
            rng = np.random.default_rng(9000 + 131 * bs + D)
            p = bm_rand_params(rng, bs, D)
            if bs <= 9:
                # (a threshold of 200 rejects every pixel of these pairs at 5x5 and 9x9: an all-invalid map)
                p["texture_threshold"] = min(p["texture_threshold"], 10)
            if (bs, D) == (9, 64):
                p.update(disp12_max_diff=1, speckle_window_size=30, speckle_range=2, uniqueness_ratio=5,
                         texture_threshold=10)
            add(f"bm-tile-bs{bs}-D{D}", "gen", "bm", _switches(("bm-tile",)), p, 1, D + 100, bs + 24, "rand_pair", bm2=0)

    # ---- 4. where the L->R lines run -----------------------------------------------------
    for aux in (0, 1, 2):
        sw = _switches(lines_aux=aux, path_sched=1)
        common = dict(family=PACKED16, sched=1, cost2=1, cost_ty=16, lines_aux=aux, stg=1)
        add(f"lines{aux}-nib-res", "lines", "sgbm", sw, sgbm_params(64, 5, mode=1, uniq=10), 3, 260, 70, "rand_pair",
            residual=1, acc=NIB, nplanes=3, nw=1, lpc=16, waves=8, ppc=0, **common)
        add(f"lines{aux}-u16", "lines", "sgbm", sw, sgbm_params(64, 9, *WIDE, mode=1, uniq=5), 3, 260, 70, "synth_pair",
            residual=0, acc=U16, nplanes=3, nw=0, lpc=16, waves=8, ppc=0, **common)
        # D 256, P 8 / 96: the no-wrap strips on plain (u16) planes
        add(f"lines{aux}-D256-nw", "lines", "sgbm", sw, sgbm_params(256, 9, 8, 96, mode=1, uniq=0), 3, 330, 70,
            "rand_pair", residual=0, acc=U16, nplanes=3, nw=1, lpc=32, waves=8, ppc=128, **common)
        add(f"lines{aux}-mode0", "lines", "sgbm", sw, sgbm_params(128, 7, mode=0, uniq=10), 3, 260, 70, "rand_pair",
            residual=1, acc=NIB, nplanes=2, nw=1, lpc=16, waves=8, ppc=64, **common)

    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


def case(name):
    return next(c for c in all_cases() if c.name == name)


def names(group):
    return [c.name for c in all_cases() if c.group == group]


def check_line(c, cus=CUS):
    """The case as a line of tests/cpp/kernel_forms_check.cpp's input (SGBM and colour cases)."""
    p = c.params
    v = [c.opts[f] for f in OPTION_FIELDS]
    v += [p["min_disparity"], p["num_disparities"], p["block_size"], p["p1"], p["p2"], p["pre_filter_cap"],
          p["uniqueness_ratio"], p["mode"], 3 if c.kind == "bgr" else 1, c.n, c.W, c.H, cus]
    return " ".join(str(int(x)) for x in v)


def frames(c, batch=0):
    """The case's n different input pairs (batch: another set of the same shape): grey uint8
    (H, W) pairs; a "bgr" case's colour pair is made from them by the test."""
    from tests.test_gpu_parity import rand_pair
    out = []
    minD, D = c.params["min_disparity"], c.params["num_disparities"]
    for k in range(c.n):
        s = 100000 * (batch + 1) + 100 * c.seed + k
        if c.recipe == "synth_pair":
            import mvstereovision3_amd as mvsv
            out.append(mvsv.synth_pair(s, c.W, c.H, max(minD, 0), D))
        else:
            # the true disparity in one of the four quarters of the range, the largest disparity
            # included (the last lanes of the path kernels), a few steps below the quarter's top
            rng = np.random.default_rng(s)
            top = minD + D - 1 - ((c.seed + k + batch) % 4) * (D // 4)
            shift = max(top - int(rng.integers(0, 3)), 0)
            out.append(rand_pair(rng, c.H, c.W, shift, (c.seed + k + batch) % 3))
    return out
