#!/usr/bin/env python3
"""Developer probe: host-side cost of the host-pointer pipeline, for A/Bs of two builds (BJJ_LIB_PATH selects the library, one
process per build and round, interleaved): bjj_mul_fixed_base on 2^20 items in pinned and in pageable memory, and on ONE item in
pinned memory, where the host's share of the call is largest.  Prints one line: ABROW {row: {median_us, min_us}}."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import babyjubjub_rs_amd as bjj
from babyjubjub_rs_amd import workload as w
c = bjj.Context(0)
n = 1 << 20
sc = np.ascontiguousarray(w.scalars_254(n)).reshape(-1)
p_in, p_out = c.host_empty(n * 32), c.host_empty(n * 64)
p_in[:] = sc
out_pg = np.zeros(n * 64, np.uint8)
def timed(fn, reps, warm):
    for _ in range(warm): fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    t.sort()
    return {"median_us": t[len(t) // 2] * 1e6, "min_us": t[0] * 1e6}
f = c.lib.bjj_mul_fixed_base
h = c.handle
a_in, a_out, s_in, s_out = p_in.ctypes.data, p_out.ctypes.data, sc.ctypes.data, out_pg.ctypes.data
def call(i, cnt, o):
    rc = f(h, i, cnt, o)
    assert rc == 0, rc
res = {}
res["fb_2p20_pinned"] = timed(lambda: call(a_in, n, a_out), 40, 8)
res["fb_2p20_pageable"] = timed(lambda: call(s_in, n, s_out), 20, 4)
res["fb_1_pinned"] = timed(lambda: call(a_in, 1, a_out), 3000, 200)
assert (np.asarray(p_out) == out_pg).all()
print("ABROW " + json.dumps(res))
c.close()
