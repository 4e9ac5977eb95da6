"""How the Panda engine launches a step, without a GPU: csrc/pbre_step_plan.hpp (plan_step, StepKnobs::from_env) compiled by the host
compiler (tests/step_plan_host) and held, launch form by launch form, to values worked out BY HAND from the rules of the launcher as it
was before the planner was split out of it (launch_step_t in csrc/pbre_panda.hpp) -- not taken from the planner.  The arithmetic is
written out beside each case.  Unless stated: NB = 2, 1024 SIMDs, default knobs, cube, MODE_STEP (fusable), blocks = ceil(n / 64)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOBS = ["rc_first_min", "idle_touch", "idle_single", "row_max", "pair", "tail_pair", "fast3", "fused", "ksample", "zero_copy", "objv_seq0"]
DEFAULTS = dict(rc_first_min=1, idle_touch=16, idle_single=1, row_max=4096, pair=2, tail_pair=0, fast3=2, fused=1, ksample=8, zero_copy=3, objv_seq0=0)
QUERY = ["n", "n_simd", "nb", "hint", "recent", "cfg_flags", "step_flags", "rt", "inner", "fusable", "obj_iso", "obj_shape", "action_repeat",
         "have_pair_g", "launches"]
QUERY0 = dict(n=131072, n_simd=1024, nb=2, hint=0, recent=0, cfg_flags=0, step_flags=0, rt=0, inner=0, fusable=1, obj_iso=1, obj_shape=0,
              action_repeat=1, have_pair_g=1, launches=0)
PLAN = ["form", "rows", "pair", "rblocks", "ntail", "fast3", "single", "rc_first", "touch_side", "rc_on_caller", "fast_on_caller", "fork_join",
        "grid_fused", "threads_fused", "grid_rc", "threads_rc", "grid_fast", "threads_fast"]
FUSED_PAIR, FUSED_64, FUSED_64_TAIL, TWO_KERNELS = 0, 1, 2, 3
NO_OBJECT, COMPLEX_ROWS, COMPLEX_LANES = 1, 8, 16      # include/pbre.h: PBRE_F_*


@pytest.fixture(scope="module")
def host():
    d = os.path.join(ROOT, "tests", "step_plan_host")
    subprocess.check_call(["make", "-s", "-C", d])
    lib = C.CDLL(os.path.join(d, "build", "libpbre_step_plan_host.so"))
    lib.step_plan.restype = None
    lib.step_knobs.restype = None
    return lib


def plan(host, **kw):
    knobs = dict(DEFAULTS, **{k: kw.pop(k) for k in list(kw) if k in DEFAULTS})
    query = dict(QUERY0, **kw)
    assert set(query) == set(QUERY), sorted(set(query) - set(QUERY))
    out = (C.c_int * len(PLAN))()
    host.step_plan((C.c_int * len(KNOBS))(*[int(knobs[k]) for k in KNOBS]), (C.c_int * len(QUERY))(*[int(query[k]) for k in QUERY]), out)
    return dict(zip(PLAN, out))


def check(p, **want):
    got = {k: p[k] for k in want}
    assert got == {k: int(v) for k, v in want.items()}, p


def knobs_of(host, from_env):
    out = (C.c_int * len(KNOBS))()
    host.step_knobs(int(from_env), out)
    return dict(zip(KNOBS, out))


# ---------------------------------------------------------------------------------------------- the step as one launch
def test_a_fresh_full_batch_is_one_64_thread_grid(host):
    # blocks 2048; pair: 2 * 2048 = 4096 > 2 * 1024; rblocks = max(64, min(256, 0 + 0 + 8)) = 64; grid 4 * 64 + 2048
    check(plan(host), form=FUSED_64, rows=1, pair=0, rblocks=64, ntail=0, grid_fused=2304, threads_fused=64)


def test_b_half_batch_is_the_pair_grid(host):
    # blocks 1024; 2 * 1024 = 2048 <= 2048: pair; grid 64 + 1024 / 2
    check(plan(host, n=65536), form=FUSED_PAIR, rows=1, pair=1, rblocks=64, ntail=0, grid_fused=576, threads_fused=256)
    # one block more does not fit two waves per SIMD: 2 * 1025 > 2048
    check(plan(host, n=65537), form=FUSED_64, pair=0, grid_fused=4 * 64 + 1025)
    # odd sizes: 100 envs = 2 chunks = 1 pair block, 129 envs = 3 chunks = 2 pair blocks
    check(plan(host, n=100), form=FUSED_PAIR, grid_fused=65)
    check(plan(host, n=129), form=FUSED_PAIR, grid_fused=66)
    # 512 SIMDs: 2048 > 1024
    check(plan(host, n=65536, n_simd=512), form=FUSED_64, pair=0)


def test_c_row_blocks_by_the_hint(host):
    # ceil(3000 / 12) = 250; coupled min(3000, 8 + 750) = 758, / 3 = 252; + 8 = 510 -> min(1024 / 4, 510) = 256; grid 4 * 256 + 2048
    check(plan(host, hint=3000), form=FUSED_64, rblocks=256, grid_fused=3072)
    # ceil(600 / 12) = 50; min(600, 158) / 3 = 52; + 8 = 110
    check(plan(host, hint=600), form=FUSED_64, rblocks=110, grid_fused=440 + 2048)
    # one complex list (NB = 1): no coupled term -- 100 + 8 against 100 + min(1200, 308) / 3 + 8 = 210
    check(plan(host, hint=1200, nb=1), rblocks=108)
    check(plan(host, hint=1200), rblocks=210)
    # 512 SIMDs: at most 128 row blocks
    check(plan(host, hint=3000, n_simd=512), rblocks=128)


def test_e_tail_pairs_by_the_hint(host):
    # rblocks 110 (above); coupled 158; 158 + ceil(442 / 4) = 111 + ceil(600 / 12) = 50 -> 319 waves; ntail = 2048 + 319 - 2048
    check(plan(host, tail_pair=1, hint=600), form=FUSED_64_TAIL, rblocks=110, ntail=319, grid_fused=440 + 2048 + 319, threads_fused=64)
    # NB = 1: 0 + ceil(600 / 4) = 150 + 50 = 200; rblocks max(64, 50 + 8) = 64
    check(plan(host, tail_pair=1, hint=600, nb=1), form=FUSED_64_TAIL, rblocks=64, ntail=200, grid_fused=256 + 2048 + 200)
    # no complex envs reported, or waves to spare (1024 + 319 - 2048 < 0): none
    check(plan(host, tail_pair=1), form=FUSED_64, ntail=0, grid_fused=2304)
    check(plan(host, tail_pair=1, hint=600, n=65536, pair=0), form=FUSED_64, ntail=0, grid_fused=440 + 1024)


def test_f_tail_pairs_by_count(host):
    check(plan(host, tail_pair=236), form=FUSED_64_TAIL, rblocks=64, ntail=236, grid_fused=256 + 2048 + 236)
    # at most blocks - 1
    check(plan(host, tail_pair=5000), form=FUSED_64_TAIL, ntail=2047, grid_fused=256 + 2048 + 2047)
    check(plan(host, tail_pair=236, n=64, pair=0), form=FUSED_64, ntail=0, grid_fused=257)
    # not with the residual exit, without the object, in an action_repeat loop, without the records
    for kw in (dict(rt=1), dict(step_flags=NO_OBJECT), dict(action_repeat=2), dict(have_pair_g=0)):
        check(plan(host, tail_pair=236, **kw), form=FUSED_64, ntail=0, grid_fused=2304, threads_fused=64)


def test_i_residual_exit_never_pairs(host):
    check(plan(host, rt=1), form=FUSED_64, pair=0, grid_fused=2304, threads_fused=64)
    for knob in (1, 2):
        check(plan(host, rt=1, n=65536, pair=knob), form=FUSED_64, pair=0, grid_fused=256 + 1024)


def test_l_settle_steps_without_the_object(host):
    # MODE 0 is fusable; blocks 256
    check(plan(host, n=16384, step_flags=NO_OBJECT), form=FUSED_64, pair=0, rblocks=64, grid_fused=512, threads_fused=64)
    check(plan(host, n=16384), form=FUSED_PAIR, pair=1, grid_fused=64 + 128)


def test_n_the_pair_knob(host):
    for n in (131072, 16384):
        blocks = n // 64
        check(plan(host, n=n, pair=0), form=FUSED_64, pair=0, grid_fused=256 + blocks)
        check(plan(host, n=n, pair=1), form=FUSED_PAIR, pair=1, grid_fused=64 + blocks // 2)
        for kw in (dict(rt=1), dict(step_flags=NO_OBJECT), dict(inner=1, fusable=0)):
            check(plan(host, n=n, pair=1, **kw), pair=0)
    check(plan(host, n=131072, pair=2), pair=0)
    check(plan(host, n=16384, pair=2), pair=1)
    check(plan(host, n=16384, pair=1, inner=1, fusable=0), form=TWO_KERNELS, threads_fast=64)


# ---------------------------------------------------------------------------------------------- which kernel steps the complex envs
def test_d_many_complex_envs_leave_the_row_kernel(host):
    # 5000 > row_max: k_fast_rc, grid min(1024, 2048 + 2); it goes first, on the caller's stream, k_fast on the side stream
    # 3-wave k_fast: 2 * ceil(5000 / 64) = 158, + 8 = 166; (2048 + 166 + 2047) / 2048 = 2 rounds > 1; 2214 <= 3 * 1024
    check(plan(host, hint=5000), form=TWO_KERNELS, rows=0, pair=0, rc_first=1, single=0, touch_side=0, rc_on_caller=1, fast_on_caller=0, fork_join=1,
          grid_rc=1024, threads_rc=64, grid_fast=2048, threads_fast=64, fast3=1)
    check(plan(host, hint=4096), form=FUSED_64, rows=1)
    check(plan(host, hint=4097), form=TWO_KERNELS, rows=0)
    check(plan(host, hint=100, row_max=99), form=TWO_KERNELS, rows=0)
    # a small batch: min(1024, 256 + 2)
    check(plan(host, n=16384, hint=5000), form=TWO_KERNELS, grid_rc=258, threads_rc=64)


def test_k_o_flag_overrides_in_order(host):
    # COMPLEX_ROWS beats the count
    check(plan(host, hint=5000, cfg_flags=COMPLEX_ROWS), form=FUSED_64, rows=1)
    # COMPLEX_LANES beats both ...
    check(plan(host, hint=10, cfg_flags=COMPLEX_LANES), form=TWO_KERNELS, rows=0)
    check(plan(host, hint=10, cfg_flags=COMPLEX_ROWS | COMPLEX_LANES), form=TWO_KERNELS, rows=0)
    # ... and an object that is no cube beats all of them: ceil(5000 / 12) = 417, min(5000, 1258) / 3 = 419, + 8 -> 256 blocks
    check(plan(host, hint=5000, obj_shape=1, cfg_flags=COMPLEX_LANES), form=FUSED_64, rows=1, rblocks=256, grid_fused=1024 + 2048)
    check(plan(host, hint=5000, obj_iso=0, cfg_flags=COMPLEX_LANES), form=FUSED_64, rows=1)
    check(plan(host, hint=5000, obj_shape=2), form=FUSED_64, rows=1)
    # three complex lists: the row kernel walks two at most
    for kw in (dict(), dict(cfg_flags=COMPLEX_ROWS), dict(obj_shape=1)):
        check(plan(host, nb=3, fusable=0, **kw), form=TWO_KERNELS, rows=0, grid_rc=1024)
    check(plan(host, n=16384, nb=3, fusable=0), grid_rc=259)


# ---------------------------------------------------------------------------------------------- two kernels
def test_g_idle_steps_share_the_callers_stream(host):
    for launches, touch in ((32, 1), (33, 0), (0, 1), (15, 0)):
        check(plan(host, fused=0, launches=launches), form=TWO_KERNELS, rows=1, single=1, rc_first=0, rc_on_caller=1, fast_on_caller=1, grid_rc=64, threads_rc=256,
              grid_fast=2048, threads_fast=64, fast3=0, touch_side=touch, fork_join=touch)
    check(plan(host, fused=0, launches=32, idle_touch=0), single=1, touch_side=0, fork_join=0)
    check(plan(host, fused=0, launches=32, idle_touch=5), single=1, touch_side=0, fork_join=0)
    check(plan(host, fused=0, launches=35, idle_touch=5), single=1, touch_side=1, fork_join=1)
    # rc_first_min = 0: "first" and single at once -- single wins, k_fast stays on the caller's stream
    check(plan(host, fused=0, launches=33, rc_first_min=0), single=1, rc_first=1, rc_on_caller=1, fast_on_caller=1, fork_join=0)
    # idle_single = 0: two streams, k_fast on the caller's; 3-wave k_fast as in H
    check(plan(host, fused=0, idle_single=0), single=0, rc_first=0, rc_on_caller=0, fast_on_caller=1, fork_join=1, touch_side=0, fast3=1)


def test_h_complex_envs_seen_lately(host):
    # hint 0 but recent 5: not single; 0 < rc_first_min: the complex envs' kernel on the side stream
    # 3-wave k_fast: rows: 0 + 0 + 8 = 8; (2048 + 8 + 2047) / 2048 = 2 > 1; 2056 <= 3072
    check(plan(host, fused=0, recent=5), form=TWO_KERNELS, single=0, rc_first=0, rc_on_caller=0, fast_on_caller=1, fork_join=1, touch_side=0, fast3=1,
          grid_rc=64, threads_rc=256, grid_fast=2048, threads_fast=64)


def test_j_inner_steps_of_action_repeat(host):
    # MODE_INNER: not fusable, never the pair kernel; 40 >= rc_first_min
    check(plan(host, n=16384, inner=1, fusable=0, hint=40, recent=16, action_repeat=2), form=TWO_KERNELS, rows=1, pair=0, rc_first=1, single=0, rc_on_caller=1,
          fast_on_caller=0, fork_join=1, grid_rc=64, threads_rc=256, grid_fast=256, threads_fast=64, fast3=0)
    check(plan(host, n=16384, inner=1, fusable=0, hint=40, recent=16, rc_first_min=41), rc_first=0, rc_on_caller=0, fast_on_caller=1, fork_join=1)


def test_m_small_batch_pair_kernel_on_the_side_stream(host):
    # pair: 2 * 256 <= 2048; rblocks = max(64, 4 + min(40, 18) / 3 + 8 = 18); 3-wave: 10 + 4 + 8 = 22 waves fit the first round
    check(plan(host, n=16384, hint=40, recent=16, fused=0), form=TWO_KERNELS, rows=1, pair=1, rblocks=64, grid_rc=64, threads_rc=256, grid_fast=256, threads_fast=128,
          rc_first=1, rc_on_caller=1, fast_on_caller=0, fork_join=1, fast3=0)
    # decided whether or not the pair kernel overrides it (the launcher counts a 3-wave step only when k_fast runs)
    check(plan(host, n=16384, hint=40, recent=16, fused=0, fast3=1), pair=1, fast3=1)


def test_the_3_wave_estimate_and_its_bounds(host):
    # rows, 2032 blocks: hint 24 -> 6 + 2 + 8 = 16 waves, 2048 in all: one round; hint 25 -> 7 + 3 + 8 = 18: a second round
    check(plan(host, n=130048, fused=0, hint=24), rows=1, fast3=0)
    check(plan(host, n=130048, fused=0, hint=25), rows=1, fast3=1)
    # k_fast_rc: hint 32512 -> 2 * 508 + 8 = 1024 waves, 3072 in all <= 3 * 1024; hint 32513 -> 1026: too many for three per SIMD
    check(plan(host, hint=32512), rows=0, fast3=1)
    check(plan(host, hint=32513), rows=0, fast3=0)
    # the knob: 0 never, 1 whenever the step is not single and has no residual exit
    check(plan(host, hint=5000, fast3=0), fast3=0)
    check(plan(host, n=16384, fused=0, pair=0, hint=40, fast3=1), fast3=1)
    check(plan(host, fused=0, fast3=1), single=1, fast3=0)
    check(plan(host, hint=5000, rt=1), form=TWO_KERNELS, fast3=0)
    check(plan(host, hint=5000, rt=1, fast3=1), fast3=0)


def test_fused_knob_and_modes_without_a_fused_kernel(host):
    check(plan(host, fused=0, hint=40), form=TWO_KERNELS, rows=1, grid_rc=64)
    check(plan(host, fusable=0, hint=40), form=TWO_KERNELS, rows=1)
    check(plan(host, hint=40), form=FUSED_64)


# ---------------------------------------------------------------------------------------------- the knobs
ENV = dict(rc_first_min="PBRE_RC_FIRST_MIN", idle_touch="PBRE_IDLE_TOUCH", idle_single="PBRE_IDLE_SINGLE", row_max="PBRE_ROW_MAX", pair="PBRE_PAIR",
           tail_pair="PBRE_TAIL_PAIR", fast3="PBRE_FAST3", fused="PBRE_FUSED", ksample="PBRE_KSAMPLE", zero_copy="PBRE_ZERO_COPY", objv_seq0="PBRE_OBJV_SEQ0")


def test_knobs_from_the_environment(host, monkeypatch):
    assert set(ENV) == set(KNOBS)
    for var in ENV.values():
        monkeypatch.delenv(var, raising=False)
    assert knobs_of(host, False) == DEFAULTS
    assert knobs_of(host, True) == DEFAULTS
    for field, var in ENV.items():
        for value in ("7", "0", "2147483646"):
            monkeypatch.setenv(var, value)
            want = dict(DEFAULTS, **{field: int(value)})
            if field == "ksample":
                want[field] = max(1, int(value))
            assert knobs_of(host, True) == want, (var, value)
        monkeypatch.delenv(var)
    assert knobs_of(host, True) == DEFAULTS
