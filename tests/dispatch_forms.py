"""Which kernel a directed test of the C ABI ran.  Calls below the short-call thresholds (bjj_hip.hip: BJJ_VB_QUAD_MAX 2^14,
BJJ_FB_QUAD_MAX 2^15, BJJ_P5_COOP_MAX 2^14, BJJ_SIGN_SMALL_MAX and BJJ_VERIFY_SMALL_MAX 2^13) run the kernels of
csrc/k_small.hip -- several lanes per item, an arithmetic of their own -- and not the one-item-per-lane kernels K1, K2, K4 and
friends that the large calls and the benchmark run.  A directed test of a few hundred items therefore sees ONE of the two unless
it asks for both: `lane_ctx` is a context whose thresholds are all 0 (read from the environment at bjj_init, as
tests/test_gpu_small_calls.py does per entry point), and `ran` asserts by bjj_info's last_* fields which form the last call took.
A plain helper module: tests import the fixture by name."""
import os

import pytest

LANE_ENV = ("BJJ_VB_QUAD_MAX", "BJJ_FB_QUAD_MAX", "BJJ_P5_COOP_MAX", "BJJ_SIGN_SMALL_MAX", "BJJ_VERIFY_SMALL_MAX")
# kind -> (bjj_info field, the value of the short-call form, the values of the one-item-per-lane forms)
FORMS = dict(fixed=("last_fixed_base_shape", 2, (0, 1)), var=("last_var_base_form", 2, (0, 1)), poseidon=("last_poseidon_form", 1, (0,)),
             sign=("last_sign_form", 1, (0,)), verify=("last_verify_dispatch", 2, (0, 1)))
SHORT, LANE = "short", "lane"


def make_lane_ctx(window_bits=16):
    import babyjubjub_rs_amd as bjj
    old = {k: os.environ.get(k) for k in LANE_ENV}
    os.environ.update({k: "0" for k in LANE_ENV})
    try:
        return bjj.Context(0, window_bits)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def lane_ctx():
    """a context whose short calls still run the one-item-per-lane kernels; 16-bit windows: no second large table"""
    c = make_lane_ctx()
    yield c
    c.close()


def ran(ctx, kind, form):
    """assert that the context's last call of that kind took the short-call form (SHORT) or a one-item-per-lane form (LANE)"""
    field, short, lane = FORMS[kind]
    got = getattr(ctx.info(), field)
    assert (got == short) if form == SHORT else (got in lane), (field, got, form)


def both(gpu_ctx, lane_ctx):
    """(context, form) for a call below the short-call thresholds: the session's context, then the lane context"""
    return ((gpu_ctx, SHORT), (lane_ctx, LANE))
