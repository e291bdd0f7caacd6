#!/usr/bin/env python3
"""Time the batched provers (tns_twist_prove_batch_device, tns_shout_prove_batch_device;
csrc/prove_batch.hip, folds in csrc/zero_folds.hip) against the only route there was before -- a loop of tns_twist_prove_device /
tns_shout_prove_device over the same resident rows -- on one GPU: n_ops in 2^8 .. 2^14 x batch in
{16, 256}.  Same process, the two interleaved, one warm-up each, the mean of --reps calls.  The
loop is the yardstick: wherever the shipped rule (csrc/prove_batch_plan.hpp) takes the batched
route, the batched call must be faster than the loop on the same box.  Also per cell: the call's
own wall-clock split (commitments, host transcripts, folds and openings: tns_last_prove_timing) and
the stage times of one profiled batched call.  One JSON line on stdout.

    python tools/prove_batch_bench.py [--logs 8,10,12,14] [--batches 16,256] [--reps 5]
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

STAGES = ["msm_batch_bits", "msm_sort", "msm_accumulate", "msm_fixup", "msm_reduce", "msm_batch_finish", "open_scan",
          "open_batch_prep", "sumcheck_round"]


class RowView:
    """one row of a resident batch, as the single provers' resident helpers take it"""

    def __init__(self, ptr):
        self.ptr = ptr


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def same(a, b, batch):
    return all(bytes(a[i]) == bytes(b[i]) for i in range(batch))


def measure(ctx, loop, batched, batch, reps):
    """warm-up of both (and the proofs agree), then `reps` interleaved calls of each"""
    want, got = loop(), batched()
    ok = same(want, got, batch)
    t_loop, t_batch = [], []
    for _ in range(reps):
        t_loop.append(timed(loop)[0])
        t_batch.append(timed(batched)[0])
    split = ctx.timing()  # of the last batched call
    ts.profile_enable(ctx, True)
    wall, _ = timed(batched)
    st = {s: ts.profile_read_ex(ctx, s) for s in STAGES}
    ts.profile_enable(ctx, False)
    rec = {"loop_s": round(sum(t_loop) / reps, 6), "batch_call_s": round(sum(t_batch) / reps, 6),
           "loop_runs_s": [round(x, 6) for x in t_loop], "batch_runs_s": [round(x, 6) for x in t_batch],
           "proofs_agree": bool(ok),
           "call_split_ms": {k: round(split[k], 3) for k in ("commit", "sumcheck", "open", "total")},
           "host_transcripts_share": round(split["sumcheck"] / split["total"], 4) if split["total"] else None,
           "profiled_wall_s": round(wall, 6),
           "stages": {s: {"ms": round(r["ms"], 4), "scopes": r["launches"]} for s, r in st.items() if r["launches"]}}
    rec["speedup"] = round(rec["loop_s"] / rec["batch_call_s"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="8,10,12,14")
    ap.add_argument("--batches", default="16,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--protocols", default="twist,shout")
    args = ap.parse_args()
    logs = [int(x) for x in args.logs.split(",")]
    batches = [int(x) for x in args.batches.split(",")]
    pp, _ = ts.setup_params(max(2, max(logs) - 2), device=args.device)  # max_operations = 2^max(logs)
    cp = pp.commitment_params
    ctx, srs = cp.srs.ctx, cp.srs
    dstate = bench.DeviceState(ts, args.device)
    dstate.start()
    rows_out = []
    for k in logs:
        n = 1 << k
        srs.prepare_lagrange(n)  # setup, not proving
        for batch in batches:
            rng = np.random.default_rng(1000 * k + batch)
            for proto in args.protocols.split(","):
                if proto == "twist":
                    addr = rng.integers(0, 1 << 20, size=(batch, n), dtype=np.uint64)
                    val = ts.fr_rand_batch(bytes([k + 1] * 32), n * batch).reshape(batch, n, 4)
                    isw = rng.integers(0, 2, size=(batch, n), dtype=np.uint8)
                    da, dv, dw = ts.DeviceBuffer(ctx, addr), ts.DeviceBuffer(ctx, val), ts.DeviceBuffer(ctx, isw)
                    views = [(RowView(da.ptr + 8 * n * b), RowView(dv.ptr + 32 * n * b), RowView(dw.ptr + n * b))
                             for b in range(batch)]
                    loop = lambda: [ts.twist_prove_resident(pp, a, v, w, n) for a, v, w in views]  # noqa: E731
                    batched = lambda: ts.twist_prove_batch_resident(pp, da, dv, dw, n, batch)  # noqa: E731
                else:
                    ent = ts.fr_rand_batch(bytes([k + 2] * 32), n * batch).reshape(batch, n, 4)
                    idx = rng.integers(0, n, size=(batch, n), dtype=np.uint64)
                    de, di = ts.DeviceBuffer(ctx, ent), ts.DeviceBuffer(ctx, idx)
                    views = [(RowView(de.ptr + 32 * n * b), RowView(di.ptr + 8 * n * b)) for b in range(batch)]
                    loop = lambda: [ts.shout_prove_resident(pp, e, n, i, n) for e, i in views]  # noqa: E731
                    batched = lambda: ts.shout_prove_batch_resident(pp, de, n, di, n, batch)  # noqa: E731
                rec = {"protocol": proto, "log_n": k, "batch": batch}
                rec.update(measure(ctx, loop, batched, batch, args.reps))
                rows_out.append(rec)
                print(json.dumps(rec), file=sys.stderr, flush=True)
    dstate.stop()
    cond = {"batched_call_beats_loop_in_every_cell": all(r["batch_call_s"] < r["loop_s"] for r in rows_out),
            "proofs_agree_in_every_cell": all(r["proofs_agree"] for r in rows_out)}
    print(json.dumps({"measured": rows_out, "conditions": cond, "reps": args.reps,
                      "note": "every cell lies on the batched route of the shipped rule (rows below the MSM batch "
                              "crossover, batch >= 2, N >= 2, a whole SRS with its Lagrange bases)",
                      "device_state": dstate.record()}), flush=True)


if __name__ == "__main__":
    main()
