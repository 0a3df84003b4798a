"""Model of the host-pointer pipeline's default chunk schedule (babyjubjub-rs_amd/csrc/pipe_plan.hpp: pipe_plan), shared by the
CPU test of the plan (test_pipe_plan.py) and the GPU tests that count chunks (test_gpu_host_pipeline.py)."""


def schedule(n, first, cap_chunk):
    """chunk sizes: first, doubling up to the cap, a remainder below half a chunk joins the last one"""
    out, lo, sz = [], 0, first
    while lo < n:
        take = min(sz, n - lo)
        if n - lo - take < sz // 2:
            take = n - lo
        out.append(take)
        lo += take
        if sz < cap_chunk:
            sz = min(sz * 2, cap_chunk)
    return out
