#!/usr/bin/env python3
"""Time the all-index vector-commitment opening (tns_vc_open_all_device, vc_open.hip) at
n = 2^12, 2^14, 2^16, 2^18, 2^20 on one GPU: the one-time tns_srs_prepare_open_all, the per-call
time on a resident vector (mean of 3 calls after one warm-up), and for comparison the only route
there was before -- one tns_vc_open per index: the mean of 16 calls times n, an EXTRAPOLATION.
Checks the two conditions the algorithm implies (n log n growth from 2^16 to 2^18; faster than the
extrapolated per-index route at 2^16).  One JSON line on stdout.

    python tools/vc_open_all_bench.py [--logs 12,14,16,18,20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multilinear-map-cryptography_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import bench  # noqa: E402
import twist_and_shout as ts  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="12,14,16,18,20")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    logs = [int(x) for x in args.logs.split(",")]
    dstate = bench.DeviceState(ts, args.device)
    dstate.start()
    pts = []
    for k in logs:
        n = 1 << k
        pp, _ = ts.setup_params(max(2, k - 2), device=args.device)  # 4 * 2^L + 1 >= n points
        cp = pp.commitment_params
        ctx = cp.srs.ctx
        cp.srs.prepare_lagrange(n)  # the basis is its own setup step
        t0 = time.perf_counter()
        cp.srs.prepare_open_all(n)
        t_prep = time.perf_counter() - t0
        vec = ts.fr_rand_batch(bytes([k] * 32), n)
        d_vec = ts.DeviceBuffer(ctx, vec)
        d_out = ts.DeviceBuffer(ctx, np.zeros((n, 8), dtype=np.uint64))
        ts.vc_open_all_resident(cp, d_vec, n, d_out)  # warm-up
        calls = []
        for _ in range(3):
            t0 = time.perf_counter()
            ts.vc_open_all_resident(cp, d_vec, n, d_out)
            calls.append(time.perf_counter() - t0)
        got = np.zeros((n, 8), dtype=np.uint64)
        ts.buffer_download(d_out, got)
        idx = [(i * (n // 16) + i) % n for i in range(16)]
        ts.KZGVectorCommitment.open(cp, vec, idx[0])  # warm-up (window table, weights)
        single, ok = [], True
        for i in idx:
            t0 = time.perf_counter()
            _, pi = ts.KZGVectorCommitment.open(cp, vec, i)
            single.append(time.perf_counter() - t0)
            x, y = (0, 0) if pi.proof is None else pi.proof
            ok = ok and ts.from_mont(got[i, :4], ts.P_MOD)[0] == x and ts.from_mont(got[i, 4:], ts.P_MOD)[0] == y
        t_all, t_one = sum(calls) / len(calls), sum(single) / len(single)
        pts.append({"log_n": k, "prepare_open_all_s": round(t_prep, 4), "open_all_device_s": round(t_all, 5),
                    "open_all_calls_s": [round(c, 5) for c in calls], "single_open_mean_s": round(t_one, 6),
                    "n_single_opens_EXTRAPOLATED_s": round(t_one * n, 2), "equals_single_opens_at_16_indices": ok})
        print(json.dumps(pts[-1]), file=sys.stderr, flush=True)
        del d_vec, d_out, cp, pp
    dstate.stop()
    by = {p["log_n"]: p for p in pts}
    cond = {}
    if 16 in by and 18 in by:
        g = by[18]["open_all_device_s"] / by[16]["open_all_device_s"]
        cond["growth_2e16_to_2e18"] = round(g, 2)
        cond["growth_below_8x"] = bool(g < 8)
    if 16 in by:
        cond["faster_than_n_single_opens_at_2e16"] = bool(
            by[16]["open_all_device_s"] < by[16]["n_single_opens_EXTRAPOLATED_s"])
    print(json.dumps({"measured": pts, "conditions": cond,
                      "note": "n_single_opens is 16 tns_vc_open calls' mean times n: an extrapolation",
                      "device_state": dstate.record()}), flush=True)


if __name__ == "__main__":
    main()
