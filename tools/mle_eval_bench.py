#!/usr/bin/env python3
"""Time the one-pass batched MLE evaluation (tns_mle_evaluate_batch_device; csrc/mle_eval.hip) and
the batched sum-check verifier built on it (tns_sumcheck_verify_batch_device;
csrc/sumcheck_verify.hip) on one GPU, and write profiles/mle_eval_bench.json.

Evaluation: K = 3 resident tables, nv in 8, 10 .. 22 at batch 16 and 8 .. 18 at batch 256 (the
cells of tools/sumcheck_batch_bench.py), random points.  The baseline is the route there was
before for the same work: mle_evaluate_dev's fold chain (csrc/mle.hip: nv launches through
ping-pong scratch and one synchronise) once per (instance, table) on the same resident data,
through tests/device/mleevalprobe.hip -- the code under test is never its own baseline.  Same
process, interleaved, one warm-up each; a timed sample is a window of back-to-back calls long
enough to time (--window-ms, sized from the warm-up), --reps samples a route, mean and runs kept;
the two routes' values must agree word for word.  Per cell also the achieved bytes/s --
32 K batch 2^nv bytes over the call's time -- beside the HBM peak, and the device time of the two
stages (mle_eval_eq, mle_eval_dot) from one profiled call made after the timed ones.

Verification: tns_sumcheck_verify_batch_device with and without tables at 256 x 2^8, 256 x 2^14
and 16 x 2^20 on the proofs tns_sumcheck_prove_batch_device made of the same resident tables (the
Twist-shaped composition A V - O O V + 2 O), the prover timed beside it; fresh transcripts, built
outside the timed region, for every call.  Without tables the call is the host replay alone: its
share of the checked call is reported.

Rows sweep (--sweep-cells): the dot-product stage's device time (mean of 5 profiled calls) against
the rows a thread takes, forced through the probe's limits at fixed cells -- the measurement behind
MleEvalLimits' defaults (csrc/ctx.hpp).

    python tools/mle_eval_bench.py [--reps 5] [--window-ms 40] [--out profiles/mle_eval_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multilinear-map-cryptography_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import bench  # noqa: E402
import twist_and_shout as ts  # noqa: E402
from twist_and_shout import _native as N  # noqa: E402

R = ts.R_MOD
TERMS = [(1, [0, 1]), (R - 1, [2, 2, 1]), (2, [2])]
K = 3
HBM_PEAK_TBS, HBM_ACHIEVABLE_TBS = 8.0, 6.3  # spec; a float4 copy's measured rate


class RowView:
    """one instance's table inside a resident batch, as the single prover's resident helpers take it"""

    def __init__(self, ctx, ptr, nbytes):
        self.ctx, self.ptr, self.nbytes = ctx, ptr, nbytes


def rand_table(rng, count):
    """count Montgomery Fr below r (top limb < 2^60): 2^20 random entries repeated, every entry made
    distinct by its index in the low limb (the values do not matter to the time; the two routes
    are compared on them)"""
    block = min(count, 1 << 20)
    t = rng.integers(0, 2**63, size=(block, 4), dtype=np.uint64) * np.uint64(2)
    t[:, 3] &= np.uint64((1 << 60) - 1)
    t = np.tile(t, (count // block, 1))
    t[:, 0] += np.arange(count, dtype=np.uint64)
    return t


def load_probe():
    lib = C.CDLL(os.path.join(PKG, "libtns_mleevalprobe.so"))
    lib.mleevalprobe_evaluate.restype = C.c_int
    lib.mleevalprobe_evaluate.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_uint, C.c_uint64, N.U64P,
                                          C.c_int, C.c_uint64, C.c_int, N.U64P, C.POINTER(C.c_int64)]
    lib.mleevalprobe_fold_chain.restype = C.c_int
    lib.mleevalprobe_fold_chain.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_uint, C.c_uint64, N.U64P,
                                            N.U64P]
    return lib


def windows(fn, reps, window_s, first_s):
    """reps samples of fn's time a call, each the mean over a window of back-to-back calls"""
    inner = max(1, min(500, int(window_s / max(first_s, 1e-6))))
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        out.append((time.perf_counter() - t0) / inner)
    return inner, out


def ok(st):
    if st != 0:
        raise RuntimeError("status %d: %s" % (st, N.last_error()))


def evaluation_cell(ctx, lib, nv, batch, args):
    n = 1 << nv
    rng = np.random.default_rng(1000 * nv + batch)
    bufs = [ts.DeviceBuffer(ctx, rand_table(rng, batch * n)) for _ in range(K)]
    ptrs = (C.c_void_p * K)(*[b.ptr for b in bufs])
    pts = ts.fr_rand_batch(bytes([nv, batch & 255] + [7] * 30), max(1, batch * nv))
    one, fold = np.zeros((batch * K, 4), dtype=np.uint64), np.zeros((batch * K, 4), dtype=np.uint64)
    info = (C.c_int64 * 4)()

    def run_one():
        ok(lib.mleevalprobe_evaluate(ctx.handle, ptrs, K, nv, batch, N.p64(pts), 1, 0, -1, N.p64(one), info))

    def run_fold():
        ok(lib.mleevalprobe_fold_chain(ctx.handle, ptrs, K, nv, batch, N.p64(pts), N.p64(fold)))

    first = {}
    for name, fn in (("fold", run_fold), ("one", run_one)):  # the warm-up, timed only to size the windows
        fn()
        t0 = time.perf_counter()
        fn()
        first[name] = time.perf_counter() - t0
    agree = bool(np.array_equal(one, fold))
    t_one, t_fold = [], []
    inner_one = inner_fold = 0
    for _ in range(args.reps):  # interleaved
        inner_fold, s = windows(run_fold, 1, args.window_ms / 1e3, first["fold"])
        t_fold += s
        inner_one, s = windows(run_one, 1, args.window_ms / 1e3, first["one"])
        t_one += s
    ts.profile_enable(ctx, True)  # one profiled call, after the timed ones
    run_one()
    stages = {s: ts.profile_read_ex(ctx, s) for s in ("mle_eval_eq", "mle_eval_dot")}
    ts.profile_enable(ctx, False)
    nbytes = 32 * K * batch * n
    rec = {"nv": nv, "batch": batch, "tables": K,
           "one_pass_s": round(sum(t_one) / len(t_one), 7), "fold_chain_s": round(sum(t_fold) / len(t_fold), 7),
           "one_pass_runs_s": [round(x, 7) for x in t_one], "fold_chain_runs_s": [round(x, 7) for x in t_fold],
           "calls_per_window": {"one_pass": inner_one, "fold_chain": inner_fold}, "values_agree": agree,
           "regime": info[0], "launches": info[1], "blocks": info[2], "rows_per_thread": info[3],
           "fold_chain_launches": batch * K * nv, "table_bytes": nbytes,
           "stage_device_ms": {s: round(v["ms"], 5) for s, v in stages.items()}}
    rec["speedup"] = round(rec["fold_chain_s"] / rec["one_pass_s"], 2)
    rec["one_pass_tb_per_s"] = round(nbytes / rec["one_pass_s"] / 1e12, 4)
    dot_ms = stages["mle_eval_dot"]["ms"]
    rec["dot_kernel_tb_per_s"] = round(nbytes / (dot_ms * 1e-3) / 1e12, 4) if dot_ms > 0 else None
    rec["one_pass_loses"] = bool(min(t_one) > max(t_fold))  # beyond the run-to-run spread
    return rec


def rows_sweep_cell(ctx, lib, nv, batch):
    n = 1 << nv
    rng = np.random.default_rng(nv + batch)
    bufs = [ts.DeviceBuffer(ctx, rand_table(rng, batch * n)) for _ in range(K)]
    ptrs = (C.c_void_p * K)(*[b.ptr for b in bufs])
    pts = ts.fr_rand_batch(bytes([nv, batch & 255] + [9] * 30), batch * nv)
    vals = np.zeros((batch * K, 4), dtype=np.uint64)
    info = (C.c_int64 * 4)()
    out = []
    for log_rows in range(0, min(nv - 8, 8) + 1):
        def run():
            ok(lib.mleevalprobe_evaluate(ctx.handle, ptrs, K, nv, batch, N.p64(pts), 1, 1, log_rows, N.p64(vals), info))

        run()
        run()
        ts.profile_enable(ctx, True)
        for _ in range(5):
            run()
        d = ts.profile_read_ex(ctx, "mle_eval_dot")
        ts.profile_enable(ctx, False)
        out.append({"rows_per_thread": info[3], "blocks": info[2], "regime": info[0], "dot_device_ms": round(d["ms"] / 5, 5)})
    return {"nv": nv, "batch": batch, "tables": K, "sweep": out}


def verification_cell(ctx, nv, batch, args):
    n = 1 << nv
    L = N.load()
    rng = np.random.default_rng(77 * nv + batch)
    bufs = [ts.DeviceBuffer(ctx, rand_table(rng, batch * n)) for _ in range(K)]
    ptrs = (C.c_void_p * K)(*[b.ptr for b in bufs])
    claims = [ts.SumCheck.composition_sum_resident(nv, [RowView(ctx, b.ptr + 32 * n * i, 32 * n) for b in bufs], TERMS)
              for i in range(batch)]
    cl = ts.to_mont(claims)
    tt = ts.SumCheck._terms(TERMS)
    rounds = np.zeros((batch * nv, 4, 4), dtype=np.uint64)
    fin = np.zeros((batch, 4), dtype=np.uint64)
    ch = np.zeros((batch * nv, 4), dtype=np.uint64)
    vch = np.zeros((batch * nv, 4), dtype=np.uint64)
    nch = np.zeros(batch, dtype=np.uint32)
    verdicts = np.zeros(batch, dtype=np.int32)
    vals = np.zeros((batch * K, 4), dtype=np.uint64)

    def transcripts():
        trs = [ts.Transcript(bytes(32)) for _ in range(batch)]
        for i, t in enumerate(trs):
            t.append_field_element(b"instance", i + 1)
        return trs, (C.c_void_p * batch)(*[t._h for t in trs])

    def prove():
        trs, handles = transcripts()
        t0 = time.perf_counter()
        ok(L.tns_sumcheck_prove_batch_device(ctx.handle, ptrs, K, nv, batch, N.p64(cl), tt, len(TERMS), handles,
                                             N.p64(rounds), N.p64(fin), N.p64(ch)))
        return time.perf_counter() - t0

    def verify(with_tables):
        trs, handles = transcripts()
        t0 = time.perf_counter()
        ok(L.tns_sumcheck_verify_batch_device(ctx.handle, ptrs if with_tables else None, K, nv, batch, N.p64(cl), tt,
                                              len(TERMS), handles, N.p64(rounds.reshape(-1, 4)), N.p64(fin), N.p64(vch),
                                              nch.ctypes.data_as(C.POINTER(C.c_uint32)),
                                              verdicts.ctypes.data_as(C.POINTER(C.c_int)),
                                              N.p64(vals) if with_tables else None))
        dt = time.perf_counter() - t0
        if verdicts.any() or not np.array_equal(vch, ch):
            raise RuntimeError("an honest proof did not verify")
        return dt

    prove()  # the proofs every verify call checks, and the warm-up
    verify(True)
    verify(False)
    t_p, t_v, t_r = [], [], []
    for _ in range(args.reps * 3):  # (short calls: three times the samples)
        t_p.append(prove())
        t_v.append(verify(True))
        t_r.append(verify(False))

    def mean(x):
        return sum(x) / len(x)

    rec = {"nv": nv, "batch": batch, "tables": K, "prove_s": round(mean(t_p), 7), "verify_with_tables_s": round(mean(t_v), 7),
           "verify_without_tables_s": round(mean(t_r), 7), "prove_runs_s": [round(x, 7) for x in t_p],
           "verify_with_tables_runs_s": [round(x, 7) for x in t_v],
           "verify_without_tables_runs_s": [round(x, 7) for x in t_r]}
    rec["host_replay_share_of_verify"] = round(rec["verify_without_tables_s"] / rec["verify_with_tables_s"], 3)
    rec["prove_over_verify"] = round(rec["prove_s"] / rec["verify_with_tables_s"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs16", default="8,10,12,14,16,18,20,22")
    ap.add_argument("--logs256", default="8,10,12,14,16,18")
    ap.add_argument("--verify-cells", default="8x256,14x256,20x16")
    ap.add_argument("--sweep-cells", default="12x256,14x256,18x256,16x16,18x16,22x16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mle_eval_bench.json"))
    args = ap.parse_args()
    ctx = ts.Context.get(args.device)
    lib = load_probe()
    dstate = bench.DeviceState(ts, args.device)
    dstate.start()
    cells = []
    for batch, logs in ((16, args.logs16), (256, args.logs256)):
        for nv in [int(x) for x in logs.split(",") if x]:
            rec = evaluation_cell(ctx, lib, nv, batch, args)
            cells.append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
    vcells = []
    for cell in [c for c in args.verify_cells.split(",") if c]:
        nv, batch = (int(x) for x in cell.split("x"))
        rec = verification_cell(ctx, nv, batch, args)
        vcells.append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    sweeps = []
    for cell in [c for c in args.sweep_cells.split(",") if c]:
        nv, batch = (int(x) for x in cell.split("x"))
        rec = rows_sweep_cell(ctx, lib, nv, batch)
        sweeps.append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    dstate.stop()
    result = {"evaluation": {"what": "K = 3 resident tables, random points; one_pass = tns_mle_evaluate_batch_device's "
                                     "internal entry, fold_chain = mle_evaluate_dev once per (instance, table)",
                             "measured": cells, "reps": args.reps, "window_ms": args.window_ms,
                             "hbm_peak_tb_per_s": HBM_PEAK_TBS, "hbm_achievable_tb_per_s": HBM_ACHIEVABLE_TBS,
                             "values_agree_in_every_cell": all(r["values_agree"] for r in cells),
                             "cells_where_one_pass_loses": [[r["nv"], r["batch"]] for r in cells if r["one_pass_loses"]]},
              "verification": {"what": "A V - O O V + 2 O (3 tables, degree 3), resident tables; the proofs of "
                                       "tns_sumcheck_prove_batch_device verified by tns_sumcheck_verify_batch_device",
                               "measured": vcells, "samples": args.reps * 3},
              "rows_sweep": {"what": "mle_eval_dot device ms against the rows a thread takes (forced limits, "
                                     "min_blocks 1), K = 3 resident tables", "measured": sweeps},
              "device_state": dstate.record()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
