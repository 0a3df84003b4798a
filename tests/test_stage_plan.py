"""The layout of the staged host forms (babyjubjub-rs_amd/csrc/stage_plan.hpp: a scratch prefix, then the arrays of one call, each at
the next multiple of 256) as pure functions on the CPU: tests/emul/emul_stage_plan.cpp, built with AddressSanitizer and UBSan and run
directly, prints the plan of every case below.  Each of the nine entries that stage a call is declared here with its array widths, and
its plan is compared with the layout computed here, with the invariants every plan has, and with the byte count the entry allocated
when it still did the arithmetic by hand: the OLD_TOTAL functions are that arithmetic, copied, and are the record of the old layout."""
import json
import os

import pytest

import hostbuild
from conftest import ROOT

COUNTS = (0, 1, 3, 4, 5, 255, 256, 257, (1 << 32) - 1)     # the last one: count * width does not fit 32 bits
SEGMENTS = (1, 3, 4, 33)                                   # m of the CSR forms
PREFIXES = (1 << 16, 5 << 20)                              # bytes of a kernel layout (MsmLayout / PointSumLayout: multiples of 256)
MAX_ARRAYS = 9


def up256(v):
    return (v + 255) // 256 * 256


# ---- what each entry allocated before the plan: its own arithmetic, one line each (L = the kernel layout's bytes) -----------------------
OLD_TOTAL = {
    "bjj_msm": lambda L, n: (L + up256(n * 64)) + up256(n * 32),                                     # o_sc + up256(n * 32)
    "bjj_msm_batch": lambda L, n, m: (L + up256(n * 64)) + up256(n * 32),                            # the same function ran both
    "bjj_mul_bases": lambda n, t: t * up256(n * 32) + n * 64,                                        # o_out + n * 64
    "verify_signer": lambda n: up256(n * 64) + up256(n * 32) + up256(n * 32) + n,                    # o_ok + n
    "verify_set": lambda n: up256(n * 64) + up256(n * 32) + up256(n * 32) + up256(n * 4) + n,        # o_ok + n
    "bjj_dlog": lambda n: up256(n * 64) + up256(n * 8) + n,                                          # o_ok + n
    "bjj_point_sum": lambda L, n, m, neg: L + up256((m + 1) * 8) + up256(n * 64) + up256(n if neg else 0) + up256(m * 64) + up256(m * 8),
    "mul_common": lambda n, add, point: up256(n * 64) + up256(n * 64 if add else 0) + up256(n * 64 if point else 0) + n,   # o_ok + n
    "bjj_elgamal_decrypt": lambda n: up256(n * 64) + up256(n * 64) + up256(n * 8) + n,               # o_ok + n
}


def site_cases():
    """(site, prefix, round_last, arrays, old total); an array is (kind, count or offset, width or bytes, present)"""
    i = lambda count, width, present=True: ("i", count if present else 0, width, present)
    o = lambda count, width, present=True: ("o", count if present else 0, width, present)
    out = []
    for n in COUNTS:
        for L in PREFIXES:
            out.append(("bjj_msm", L, 1, [i(n, 64), i(n, 32), ("O", 4096, 64, True), ("O", 256, 8, True)], OLD_TOTAL["bjj_msm"](L, n)))
            for m in SEGMENTS:
                out.append(("bjj_msm_batch", L, 1, [i(n, 64), i(n, 32), ("I", 1024, (m + 1) * 8, True), ("O", 4096, m * 64, True), ("O", 256, m * 8, True)],
                            OLD_TOTAL["bjj_msm_batch"](L, n, m)))
                for neg in (False, True):
                    out.append(("bjj_point_sum", L, 1, [i(m + 1, 8), i(n, 64), i(n, 1, neg), o(m, 64), o(m, 8)], OLD_TOTAL["bjj_point_sum"](L, n, m, neg)))
        for t in range(1, 9):
            out.append(("bjj_mul_bases", 0, 0, [i(n, 32)] * t + [o(n, 64)], OLD_TOTAL["bjj_mul_bases"](n, t)))
        out.append(("verify_signer", 0, 0, [i(n, 64), i(n, 32), i(n, 32), o(n, 1)], OLD_TOTAL["verify_signer"](n)))
        out.append(("verify_set", 0, 0, [i(n, 64), i(n, 32), i(n, 32), i(n, 4), o(n, 1)], OLD_TOTAL["verify_set"](n)))
        out.append(("bjj_dlog", 0, 0, [i(n, 64), o(n, 8), o(n, 1)], OLD_TOTAL["bjj_dlog"](n)))
        for add in (False, True):
            for point in (False, True):                    # bjj_in_subgroup has no result array
                out.append(("mul_common", 0, 0, [i(n, 64), i(n, 64, add), o(n, 64, point), o(n, 1)], OLD_TOTAL["mul_common"](n, add, point)))
        out.append(("bjj_elgamal_decrypt", 0, 0, [i(n, 64), i(n, 64), o(n, 8), o(n, 1)], OLD_TOTAL["bjj_elgamal_decrypt"](n)))
    return out


def _line(prefix, round_last, arrays):
    return "%d %d %s" % (prefix, round_last, " ".join("%s:%d:%d" % a[:3] for a in arrays))


def model(prefix, round_last, arrays):
    """the layout, computed here: -> (offsets, bytes, total)"""
    end, offs, sizes = prefix, [], []
    for kind, a, b, _ in arrays:
        if kind in "IO":
            offs.append(a); sizes.append(b)
            continue
        off = up256(end)
        offs.append(off); sizes.append(a * b)
        if a * b:
            end = off + a * b
    return offs, sizes, up256(end) if round_last else end


@pytest.fixture(scope="module")
def emul():
    """run(lines) -> the program's output lines; the sanitizers abort on the first finding"""
    hostbuild.need_sanitizer_runtimes()
    exe = hostbuild.program("emul_stage_plan", os.path.join(ROOT, "tests", "emul", "emul_stage_plan.cpp"), san=True)

    def run(lines):
        text = hostbuild.run_sanitized(exe, "\n".join(lines) + "\n", timeout=300)
        out = text.splitlines()
        assert len(out) == len(lines), text[-3000:]
        return [json.loads(l) for l in out]
    return run


def test_every_site_keeps_its_layout_and_its_byte_count(emul):
    cases = site_cases()
    assert {c[0] for c in cases} == set(OLD_TOTAL) and len(OLD_TOTAL) == 9
    plans = emul([_line(prefix, rl, arrays) for _, prefix, rl, arrays, _ in cases])
    for (site, prefix, rl, arrays, old_total), p in zip(cases, plans):
        ctx = (site, prefix, arrays, p)
        offs, sizes, total = model(prefix, rl, arrays)
        assert p["idx"] == list(range(len(arrays))) and p["off"] == offs and p["bytes"] == sizes, ctx
        assert p["out"] == [int(a[0] in "oO") for a in arrays], ctx
        assert p["total"] == total == old_total, ctx                       # the entry allocates what it always did
        behind = [(off, size, a) for off, size, a in zip(p["off"], p["bytes"], arrays) if a[0] in "io"]
        at = prefix
        for off, size, a in behind:                                        # argument order, no overlap with each other or the prefix
            assert off % 256 == 0 and off >= at, ctx
            if not a[3]:
                assert size == 0, ctx                                      # an absent array
            at = max(at, off + size)
        assert at <= p["total"] and p["total"] - at < 256, ctx
        for off, size, a in zip(p["off"], p["bytes"], arrays):             # an array at a given offset lies inside the prefix
            if a[0] in "IO":
                assert off + size <= prefix, ctx


def test_an_absent_array_costs_no_space(emul):
    """the plan of a call without an optional array is the plan of the call that never had it"""
    cases = [(s, prefix, rl, arrays) for s, prefix, rl, arrays, _ in site_cases() if any(not a[3] for a in arrays)]
    assert {c[0] for c in cases} == {"bjj_point_sum", "mul_common"}
    with_it = emul([_line(prefix, rl, arrays) for _, prefix, rl, arrays in cases])
    without = emul([_line(prefix, rl, [a for a in arrays if a[3]]) for _, prefix, rl, arrays in cases])
    for (site, prefix, rl, arrays), p, q in zip(cases, with_it, without):
        keep = [k for k, a in enumerate(arrays) if a[3]]
        assert [p["off"][k] for k in keep] == q["off"] and [p["bytes"][k] for k in keep] == q["bytes"] and p["total"] == q["total"], (site, arrays)


def test_the_plan_is_full_at_nine_arrays(emul):
    """bjj_mul_bases with BJJ_MAX_BASES = 8 scalar arrays and its results is the largest site; one more is refused, nothing is written"""
    p, = emul([_line(0, 0, [("i", 5, 32, True)] * MAX_ARRAYS + [("o", 5, 64, True), ("O", 0, 8, True)])])
    assert p["idx"] == list(range(MAX_ARRAYS)) + [-1, -1] and len(p["off"]) == MAX_ARRAYS
