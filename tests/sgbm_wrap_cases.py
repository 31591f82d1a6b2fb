"""SGBM launches whose costs leave int16, over the forms the general recurrence can take (no
GPU, fixed seeds).  The sibling of tests/kernel_form_cases.py for the regime where
``sgbm_no_wrap`` is false *and the values themselves pass 32767*.

Past 32767 OpenCV's result depends on its build: the SIMD row update of the cost volume
saturates, the scalar one wraps (oracle/mvsv_oracle.h, ORC_F_COST_WRAP).  Every case names the
oracle flags it is compared under: its ``variant`` word (what the engine is given) and
``COST_FLAG`` on top of it, the update the engine reproduces.

Inputs are ``saw_pair`` (tests/test_gpu_parity.py).  In every case at least 3 % of the cost
volume is above 32767 and the two updates give maps that differ in at least 1 % of the pixels
(tests/test_sgbm_wrap_cases.py asserts these and the other input conditions on the CPU).  With
blockSize >= 17 a faded sawtooth of period 8 under noise 20 does that for any penalty.  The
register-ring cost kernel (blockSize <= 15) sums 225 pixel costs: under u16 planes P2 = 9000
carries the faded sawtooth past the limit; under nibble / byte planes (P2 <= 51) only an
unfaded sawtooth of period 28 / 29 under noise 1 / 2 gets there (window sums peak near
35 000), and which seed, shift, mode and variant word hold all the conditions was searched
per numDisparities (``SMALL_P2``).  numDisparities 256 takes 520 columns: the map's share of
valid pixels counts the 256 columns left of the cost space too.

The table is the union of the cases the forms need (``FORM_AXES``: one case per distinct plan
tuple ``form_key``; the stated form is written out by ``stated_form`` from the plan's rules
for a small launch and checked against sgbm_make_plan) and of the cases that must be there
whatever the plan says (``req``).
"""
from collections import namedtuple
from functools import lru_cache
from itertools import product

import numpy as np

from tests import kernel_form_cases as kc
from tests.kernel_form_cases import BITSLICE, GENERIC, NIB, PACKED8, PACKED16, U8, U16, sgbm_params  # noqa: F401

CUS = kc.CUS
F_FIRSTCOL_FIX, F_WTA_MIN_D, F_COST_WRAP = 1, 2, 4
# The cost-row update the engine reproduces past 32767: the oracle flag
# every case adds to its variant word.
COST_FLAG = F_COST_WRAP

Case = namedtuple("Case", "name group kind env opts params n W H recipe seed form variant saw")

# the KernelOptions fields of tests/cpp/kernel_forms_check.cpp's "wide" lines, after kc.OPTION_FIELDS
WIDE_FIELDS = ("tri32", "final_split", "strip_waves")
OPTION_DEFAULTS = dict(kc.OPTION_DEFAULTS, tri32=1, final_split=1, strip_waves=0)
ENV_INTS = dict(kc.ENV_INTS, MVSV_TRI32="tri32", MVSV_FINAL_SPLIT="final_split", MVSV_STRIP_WAVES="strip_waves")
PLAN_FIELDS = kc.PLAN_FIELDS + ("no_wrap",)
KEY_FIELDS = ("cost2", "ppc", "family", "sched", "acc", "split", "lpc", "waves")

# the axes of the plan enumeration (tests/test_sgbm_wrap_cases.py runs sgbm_make_plan over their product)
FORM_AXES = dict(D=(16, 32, 48, 64, 128, 256), mode=(0, 1), bs=(15, 21), P2=(5, 30, 3000), sched=(0, 1, 2),
                 forced=(0, 1), word=(None, "cost-lds", "cost-generic", "path-wave", "path-lines"),
                 final_split=(0, 1), tri32=(0, 1))
# P1 beside each P2 of the enumeration
P1_OF = {5: 2, 30: 8, 3000: 100}


def wide_waves(D):
    """tri_wide_waves at 16 lanes: the strip width MVSV_STRIP_WAVES forces (0: D has no strips)."""
    return {32: 15, 64: 15, 128: 15, 256: 7}.get(D, 0)


def switches(word=None, **ints):
    """(env, opts) of one choice, as kc._switches, with the three wide fields."""
    env, opts = {}, dict(OPTION_DEFAULTS)
    if word:
        env["MVSV_KERNELS"] = word
        opts[kc.KERNEL_WORDS[word]] = 0
    names = {v: k for k, v in ENV_INTS.items()}
    for field, v in ints.items():
        if v != OPTION_DEFAULTS[field]:
            env[names[field]] = str(v)
            opts[field] = v
    return env, opts


def form_key(plan):
    return tuple(int(plan[f]) for f in KEY_FIELDS)


def stated_form(D, mode, bs, P2, sched, forced, word, final_split, tri32):
    """sgbm_make_plan's rules for one small frame in the general recurrence (256 CUs: every
    schedule-by-size choice lands on "side by side", every strip launch is "few"), written
    out again; tests/test_sgbm_wrap_cases.py compares it with the header's plan."""
    cost2 = int(bs <= 15 and word != "cost-lds")
    ppc = -1 if not cost2 else 0 if word == "cost-generic" else {128: 64, 256: 128}.get(D, 0)
    path16, tri, wide = word != "path-wave", word != "path-lines", D in (32, 64, 128, 256)
    if D == 16:
        s = 2 if path16 and sched != 1 else 0
    elif not (wide and path16):
        s = 0
    else:
        s = 2 if sched in (0, 2) else 1 if tri else 0
    family = PACKED8 if D == 16 and s == 2 else PACKED16 if wide and path16 else GENERIC
    ndir = 8 if mode else 5
    acc = NIB if (s == 2 and P2 <= 15) or (s == 1 and 3 * P2 <= 15) else U8 if ndir * P2 <= 255 else U16
    split = int(s == 2 and final_split and P2 > 15 and D <= 32)
    lpc = waves = 0
    if s == 1 and family == PACKED16:
        lpc, waves = 16, (4 if D == 256 else 8)
        if D == 256 and tri32 and not forced:
            lpc, waves = 32, 8
        elif forced:
            waves = wide_waves(D)
    return dict(cost2=cost2, ppc=ppc, family=family, sched=s, acc=acc, split=split, lpc=lpc, waves=waves, nw=0,
                residual=0, no_wrap=0)


# saw_pair arguments (period, noise, shift, fade) by window and penalty
SAW_FADE = dict(period=8, noise=20, shift=3, fade=1)   # blockSize 17..21, and 15 under P2 >= 9000
# blockSize 15 under P2 <= 51, by numDisparities: saw_pair arguments with the seed, then mode, minDisparity,
# variant word, uniquenessRatio
SMALL_P2 = {
    16: (dict(period=29, noise=1, shift=6, fade=0, seed=1055), 1, -2, 0, 5),
    32: (dict(period=28, noise=2, shift=2, fade=0, seed=1025), 0, -2, 3, 0),
    64: (dict(period=29, noise=2, shift=6, fade=0, seed=1030), 0, -2, 2, 5),
    128: (dict(period=29, noise=1, shift=9, fade=0, seed=1067), 1, -2, 1, 5),
    256: (dict(period=29, noise=1, shift=3, fade=0, seed=1021), 1, -2, 3, 0),
}


def _width(D):
    return {128: 260, 256: 520}.get(D, D + 100)


@lru_cache(maxsize=None)
def all_cases():
    cs = []
    seed = [7000]

    def add(name, group, kind, sw, params, n, W, H, recipe, variant, saw, **form):
        env, opts = sw
        form.setdefault("split", 0)
        form["bits"] = kc.plan_bits(form)
        seed[0] += 1
        cs.append(Case(name, group, kind, env, opts, params, n, W, H, recipe, seed[0], form, variant, saw))

    # ---- 1. one case per plan tuple ------------------------------------------------------
    seen = set()
    ax = FORM_AXES
    for D, bs, P2, sched, forced, word, fs, t32 in product(ax["D"], (21, 15), ax["P2"], ax["sched"], ax["forced"],
                                                          ax["word"], (1, 0), (1, 0)):
        key = form_key(stated_form(D, 0, bs, P2, sched, forced, word, fs, t32))  # (the tuple holds no mode)
        if key in seen:
            continue
        seen.add(key)
        i = len(cs)
        small = bs == 15 and P2 <= 51
        if small:
            saw, mode, minD, variant, uniq = SMALL_P2[D]
            disp12 = 1
        else:
            saw, mode, minD, variant = SAW_FADE, (i // 2) % 2, (0, -2, 3)[i % 3], i % 4
            uniq, disp12 = (0, 5)[i % 2], (-1, 1)[(i // 2) % 2]
        form = stated_form(D, mode, bs, P2, sched, forced, word, fs, t32)
        assert form_key(form) == key
        # u16 planes behind the register-ring kernel: P2 9000 (OpenCV's recommended 32 * blockSize^2 is 7200)
        P1, P2e = (600, 9000) if (bs == 15 and P2 == 3000) else (P1_OF[P2], P2)
        sw = switches(word, path_sched=sched, strip_waves=wide_waves(D) if forced else 0, final_split=fs, tri32=t32)
        name = (f"{word or 'dflt'}-D{D}-bs{bs}-P{P2e}-s{sched}" + ("-wide" if forced else "") + ("" if fs else "-nosplit") +
                ("" if t32 else "-tri16") + f"-m{mode}")
        add(name, "form", "sgbm", sw, sgbm_params(D, bs, P1, P2e, cap=63, uniq=uniq, disp12=disp12, minD=minD, mode=mode),
            1, _width(D), 41, "saw_pair", variant, saw, **form)

    # ---- 2. the cases that must be there whatever the plan says ---------------------------
    def req(name, D, bs, P1, P2, mode, variant, word=None, H=41, n=1, kind="sgbm", recipe="saw_pair", saw=SAW_FADE,
            uniq=5, disp12=1, minD=0, W=None, **ints):
        sched = ints.get("path_sched", 0)
        form = stated_form(D, mode, bs, P2, sched, 0, word, 1, 1)
        if kind == "bgr":  # colour pairs always take the LDS-ring kernel
            form.update(cost2=0, ppc=-1)
        if "cost_ty" in ints:
            form["cost_ty"] = ints["cost_ty"]
        add(name, "req", kind, switches(word, **ints),
            sgbm_params(D, bs, P1, P2, cap=63, uniq=uniq, disp12=disp12, minD=minD, mode=mode), n, W or _width(D), H,
            recipe, variant, saw, **form)

    # both cost kernels: the register ring (blockSize <= 15) at D 64 / 128 / 256, the LDS ring at 17 .. 21 and,
    # by switch, at 15
    for i, D in enumerate((64, 128, 256)):
        req(f"ring-D{D}-bs15", D, 15, 600, 9000, i % 2, i, uniq=0, disp12=-1)
    for i, bs in enumerate((17, 19, 21)):
        req(f"lds-bs{bs}", 32, bs, 100, 3000, (i + 1) % 2, 3 - i, minD=(-2, 0, 3)[i])
    req("lds-bs15", 64, 15, 600, 9000, 1, 1, word="cost-lds")
    # a wrap across a tile seam: forced tile height 24 at H = 51 (rows 24 and 48), both kernels
    req("ty24-H51-ring", 64, 15, 600, 9000, 0, 3, H=51, cost_ty=24)
    req("ty24-H51-lds", 32, 21, 8, 100, 1, 0, H=51, cost_ty=24)
    # the four variant words in both modes (the column-0 and bottom-row fix-ups write C too)
    for mode in (0, 1):
        for v in range(4):
            req(f"var{v}-mode{mode}", 32, 21, 8, 100, mode, v, H=40, W=120, uniq=(0, 5)[v % 2], disp12=(-1, 1)[mode])
    # odd heights at D >= 128: the final kernel's two rows per wave
    req("odd-D128-H37", 128, 21, 8, 96, 1, 2, H=37, minD=3)
    req("odd-D256-H43", 256, 21, 8, 96, 0, 1, H=43, minD=-2)
    # double wrap (T > 65535; the window sums reach 50 000) at D 48 (the generic family), and nibble planes
    # over wrapped costs
    req("double-wrap", 48, 21, 300, 18000, 0, 0, H=25, W=110)
    req("nib-bs21", 32, 21, 2, 5, 1, 3, H=40, W=120, uniq=0)
    # without the fade: the two updates part on the noise alone
    req("nofade-D16", 16, 15, 600, 9000, 1, 0, H=30, W=100, saw=dict(period=6, noise=20, shift=3, fade=0))
    # a three-frame device batch, the middle frame a rand_pair that does not wrap: the plan is per launch,
    # the data per frame
    req("batch3-mid-plain", 64, 21, 8, 100, 1, 2, n=3, recipe="saw_rand_saw", path_sched=1)
    # one live colour channel over constant ftzero planes: the cn = 3 cost kernel on wrapped sums
    req("bgr-bs15", 64, 15, 600, 9000, 0, 1, kind="bgr")

    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


def case(name):
    return next(c for c in all_cases() if c.name == name)


def names(group=None):
    return [c.name for c in all_cases() if group is None or c.group == group]


def wide_line(opts, params, channels, n, W, H, cus=CUS):
    """One "wide" input line of tests/cpp/kernel_forms_check.cpp."""
    p = params
    v = [opts[f] for f in kc.OPTION_FIELDS]
    v += [p["min_disparity"], p["num_disparities"], p["block_size"], p["p1"], p["p2"], p["pre_filter_cap"],
          p["uniqueness_ratio"], p["mode"], channels, n, W, H, cus]
    v += [opts[f] for f in WIDE_FIELDS]
    return " ".join(str(int(x)) for x in v)


def check_line(c):
    return wide_line(c.opts, c.params, 3 if c.kind == "bgr" else 1, c.n, c.W, c.H)


def enumeration():
    """[(axes dict, wide line)] over the product of FORM_AXES, one frame of the table's shape."""
    out = []
    names_ = tuple(FORM_AXES)
    for vals in product(*FORM_AXES.values()):
        a = dict(zip(names_, vals))
        _, opts = switches(a["word"], path_sched=a["sched"], strip_waves=wide_waves(a["D"]) if a["forced"] else 0,
                           final_split=a["final_split"], tri32=a["tri32"])
        p = sgbm_params(a["D"], a["bs"], P1_OF[a["P2"]], a["P2"], cap=63, uniq=5, mode=a["mode"])
        out.append((a, wide_line(opts, p, 1, 1, _width(a["D"]), 41)))
    return out


def frames(c):
    """The case's n input pairs (grey uint8 (H, W)) and, per pair, whether it is a sawtooth."""
    from tests.test_gpu_parity import rand_pair, saw_pair
    out = []
    for k in range(c.n):
        if c.recipe == "saw_rand_saw" and k == 1:
            rng = np.random.default_rng(c.seed)
            out.append(rand_pair(rng, c.H, c.W, c.params["num_disparities"] // 2, 0) + (False,))
        else:
            out.append(saw_pair(c.H, c.W, **dict(c.saw, seed=c.saw.get("seed", 100 * c.seed) + k)) + (True,))
    return out


@lru_cache(maxsize=None)
def references(name):
    """Per frame of the case: (oracle map under variant | F_COST_WRAP, oracle map under variant) -- the wrapping
    and the saturating cost update.  Computed once, shared by the CPU and the GPU tests, never written to."""
    from oracle import pyoracle
    c = case(name)
    out = []
    for L, R, _ in frames(c):
        a = pyoracle.sgbm(L, R, c.params, c.variant | F_COST_WRAP)
        b = pyoracle.sgbm(L, R, c.params, c.variant)
        a.setflags(write=False), b.setflags(write=False)
        out.append((a, b))
    return tuple(out)
