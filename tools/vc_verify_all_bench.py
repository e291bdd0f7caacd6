#!/usr/bin/env python3
"""Time the batched verifier of a vector commitment's openings (tns_vc_verify_all_device,
kzg_verify.hip) at n = 2^12, 2^16, 2^18, 2^20 on one GPU, on tns_vc_open_all_device's own output:
the check on resident data (mean of 3 calls after one warm-up, challenges from the OS), each stage's
share of it (verify_points, verify_scalars, msm_sort, msm_accumulate), the locate path with one value
changed at n - 1, and for comparison the only sound route there was before -- one
KZGVectorCommitment.verify per index: the mean of 16 calls times n, an EXTRAPOLATION.
Checks the two conditions the algorithm implies (two pairings against 2 n: faster than the
extrapolated per-index route at 2^16; O(n) MSM work: less than 32x from 2^16 to 2^20).
One JSON line on stdout.

    python tools/vc_verify_all_bench.py [--logs 12,16,18,20]
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

STAGES = ["verify_points", "verify_scalars", "msm_sort", "msm_accumulate"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="12,16,18,20")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    logs = [int(x) for x in args.logs.split(",")]
    dstate = bench.DeviceState(ts, args.device)
    dstate.start()
    pts = []
    for k in logs:
        n = 1 << k
        pp, vp = ts.setup_params(max(2, k - 2), device=args.device)  # 4 * 2^L + 1 >= n points
        cp, vk = pp.commitment_params, vp.commitment_vk
        ctx = cp.srs.ctx
        cp.srs.prepare_lagrange(n)
        cp.srs.prepare_open_all(n)
        vec = ts.fr_rand_batch(bytes([k] * 32), n)
        cm = ts.KZGVectorCommitment.commit(cp, vec)
        d_vec = ts.DeviceBuffer(ctx, vec)
        d_pi = ts.DeviceBuffer(ctx, np.zeros((n, 8), dtype=np.uint64))
        ts.vc_open_all_resident(cp, d_vec, n, d_pi)
        ok = ts.vc_verify_all_resident(vk, cm, d_vec, n, d_pi)  # warm-up
        calls = []
        for _ in range(3):
            t0 = time.perf_counter()
            ok = ts.vc_verify_all_resident(vk, cm, d_vec, n, d_pi) and ok
            calls.append(time.perf_counter() - t0)
        ts.profile_enable(ctx, True)  # a fourth call under the stage timers (not in the mean)
        t0 = time.perf_counter()
        ok = ts.vc_verify_all_resident(vk, cm, d_vec, n, d_pi) and ok
        t_prof = time.perf_counter() - t0
        stages = {s: ts.profile_read_ex(ctx, s) for s in STAGES}
        ts.profile_enable(ctx, False)
        bad = vec.copy()
        bad[n - 1] = ts.to_mont([1])[0]
        d_bad = ts.DeviceBuffer(ctx, bad)
        t0 = time.perf_counter()
        located = ts.vc_verify_all_resident(vk, cm, d_bad, n, d_pi, locate=True)
        t_locate = time.perf_counter() - t0
        got = np.zeros((n, 8), dtype=np.uint64)
        ts.buffer_download(d_pi, got)
        vals = ts.from_mont(vec[[(i * (n // 16) + i) % n for i in range(16)]])
        single, each = [], True
        for j, i in enumerate((i * (n // 16) + i) % n for i in range(16)):
            x, y = ts.from_mont(got[i, :4], ts.P_MOD)[0], ts.from_mont(got[i, 4:], ts.P_MOD)[0]
            pi = ts.KZGProof((x, y) if got[i].any() else None)
            t0 = time.perf_counter()
            each = ts.KZGVectorCommitment.verify(vk, cm, i, vals[j], pi) and each
            single.append(time.perf_counter() - t0)
        t_all, t_one = sum(calls) / len(calls), sum(single) / len(single)
        pts.append({"log_n": k, "verify_all_device_s": round(t_all, 6),
                    "verify_all_calls_s": [round(c, 6) for c in calls], "accepted": bool(ok),
                    "profiled_call_s": round(t_prof, 6),
                    "stage_ms": {s: round(v["busy_ms"], 4) for s, v in stages.items()},
                    "stage_share_of_profiled_call": {s: round(v["busy_ms"] / (1e3 * t_prof), 4)
                                                     for s, v in stages.items()},
                    "locate_bad_value_at_last_index_s": round(t_locate, 6),
                    "located": [bool(located[0]), located[1]], "located_ok": located == (False, n - 1),
                    "single_verify_mean_s": round(t_one, 6), "single_verifies_accept": bool(each),
                    "n_single_verifies_EXTRAPOLATED_s": round(t_one * n, 2)})
        print(json.dumps(pts[-1]), file=sys.stderr, flush=True)
        del d_vec, d_pi, d_bad, cp, pp
    dstate.stop()
    by = {p["log_n"]: p for p in pts}
    cond = {}
    if 16 in by:
        cond["faster_than_n_single_verifies_at_2e16"] = bool(
            by[16]["verify_all_device_s"] < by[16]["n_single_verifies_EXTRAPOLATED_s"])
    if 16 in by and 20 in by:
        g = by[20]["verify_all_device_s"] / by[16]["verify_all_device_s"]
        cond["growth_2e16_to_2e20"] = round(g, 2)
        cond["growth_below_32x"] = bool(g < 32)
    print(json.dumps({"measured": pts, "conditions": cond,
                      "note": "n_single_verifies is 16 KZGVectorCommitment.verify calls' mean times n: an "
                              "extrapolation; stage_ms is each stage's busy time (union of its launch intervals)",
                      "device_state": dstate.record()}), flush=True)
    if not all(cond.values()) or not all(p["accepted"] and p["located_ok"] for p in pts):
        sys.exit(1)


if __name__ == "__main__":
    main()
