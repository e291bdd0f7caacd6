#!/usr/bin/env python3
"""Time the batched generic sum-check (tns_sumcheck_prove_batch_device; csrc/sumcheck_batch.hip)
against the only route there was before -- tns_sumcheck_prove_device row by row over the same
resident tables -- on one GPU: the 3-table Twist-shaped composition A V - O O V + 2 O, nv in
8 .. 20 x batch in {16, 256}, cells of more than 2^--max-log table entries left out.  Both routes
are forced through the shipped internal entry point (tests/device/scbatchprobe.hip: the rows route
is the single prover in a loop inside the library, the batched route one call), in the same
process, interleaved, one warm-up each, fresh transcripts (built outside the timed region) for
every call, the mean of --reps calls; the two routes' outputs must agree byte for byte.  The
crossover of csrc/sumcheck_batch_plan.hpp is the smallest 2^nv at which batched is not faster at
batch 16.  One JSON line on stdout.

    python tools/sumcheck_batch_bench.py [--logs 8,10,12,14,16,18,20] [--batches 16,256] [--reps 5]
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
ROWS, BATCHED = 0, 1


class RowView:
    """one instance's table inside a resident batch, as the single prover's resident helpers take it"""

    def __init__(self, ctx, ptr, nbytes):
        self.ctx, self.ptr, self.nbytes = ctx, ptr, nbytes


def rand_table(rng, count):
    """count Montgomery Fr (limbs below r: top limb < 2^60)"""
    t = rng.integers(0, 2**63, size=(count, 4), dtype=np.uint64) * np.uint64(2)
    t += rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    t[:, 3] &= np.uint64((1 << 60) - 1)
    return t


def load_probe():
    lib = C.CDLL(os.path.join(PKG, "libtns_scbatchprobe.so"))
    lib.scbatchprobe_prove.restype = C.c_int
    lib.scbatchprobe_prove.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_uint, C.c_uint64, N.U64P,
                                       C.POINTER(N.TnsTerm), C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_int,
                                       C.c_uint64, C.c_uint64, N.U64P, N.U64P, N.U64P, C.POINTER(C.c_int64)]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="8,10,12,14,16,18,20")
    ap.add_argument("--batches", default="16,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-log", type=int, default=24, help="skip cells of more than 2^this entries a table")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    logs = [int(x) for x in args.logs.split(",")]
    batches = [int(x) for x in args.batches.split(",")]
    ctx = ts.Context.get(args.device)
    lib = load_probe()
    tt = ts.SumCheck._terms(TERMS)
    dstate = bench.DeviceState(ts, args.device)
    dstate.start()
    cells, skipped = [], []
    for nv in logs:
        n = 1 << nv
        for batch in batches:
            if batch * n > 1 << args.max_log:
                skipped.append({"nv": nv, "batch": batch})
                continue
            rng = np.random.default_rng(1000 * nv + batch)
            bufs = [ts.DeviceBuffer(ctx, rand_table(rng, batch * n)) for _ in range(3)]
            ptrs = (C.c_void_p * 3)(*[b.ptr for b in bufs])
            claims = [ts.SumCheck.composition_sum_resident(nv, [RowView(ctx, b.ptr + 32 * n * i, 32 * n) for b in bufs],
                                                           TERMS) for i in range(batch)]
            cl = ts.to_mont(claims)
            rounds = np.zeros((batch * nv, 4, 4), dtype=np.uint64)
            fin = np.zeros((batch, 4), dtype=np.uint64)
            ch = np.zeros((batch * nv, 4), dtype=np.uint64)
            info = (C.c_int64 * 4)()

            def call(force):
                """(seconds, outputs, info) of one forced call on fresh transcripts"""
                trs = [ts.Transcript(bytes(32)) for _ in range(batch)]
                for i, t in enumerate(trs):
                    t.append_field_element(b"instance", i + 1)
                handles = (C.c_void_p * batch)(*[t._h for t in trs])
                t0 = time.perf_counter()
                st = lib.scbatchprobe_prove(ctx.handle, ptrs, 3, nv, batch, N.p64(cl), tt, len(TERMS), handles, 1, force,
                                            0, 0, N.p64(rounds), N.p64(fin), N.p64(ch), info)
                dt = time.perf_counter() - t0
                if st != 0:
                    raise RuntimeError("status %d: %s" % (st, N.last_error()))
                return dt, (rounds.tobytes(), fin.tobytes(), ch.tobytes()), tuple(info)

            _, want, info_rows = call(ROWS)
            _, got, info_batched = call(BATCHED)
            assert info_rows[0] == ROWS and info_batched[0] == BATCHED, (info_rows, info_batched)
            t_rows, t_batched = [], []
            for _ in range(args.reps):
                t_rows.append(call(ROWS)[0])
                t_batched.append(call(BATCHED)[0])
            rec = {"nv": nv, "batch": batch, "rows_s": round(sum(t_rows) / args.reps, 6),
                   "batched_s": round(sum(t_batched) / args.reps, 6), "rows_runs_s": [round(x, 6) for x in t_rows],
                   "batched_runs_s": [round(x, 6) for x in t_batched], "outputs_agree": want == got,
                   "group_rows": info_batched[1], "groups": info_batched[2], "launches": info_batched[3]}
            rec["rows_ms_per_instance"] = round(1e3 * rec["rows_s"] / batch, 4)
            rec["batched_ms_per_instance"] = round(1e3 * rec["batched_s"] / batch, 4)
            rec["speedup"] = round(rec["rows_s"] / rec["batched_s"], 2)
            cells.append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
            del bufs
    dstate.stop()
    lost16 = sorted(r["nv"] for r in cells if r["batch"] == 16 and not r["batched_s"] < r["rows_s"])
    print(json.dumps({"composition": "A V - O O V + 2 O (3 tables, degree 3), resident tables", "measured": cells,
                      "skipped_cells": skipped, "skipped_because": "more than 2^%d entries a table" % args.max_log,
                      "reps": args.reps,
                      "smallest_nv_where_batched_is_not_faster_at_batch_16": lost16[0] if lost16 else None,
                      "outputs_agree_in_every_cell": all(r["outputs_agree"] for r in cells),
                      "device_state": dstate.record()}), flush=True)


if __name__ == "__main__":
    main()
