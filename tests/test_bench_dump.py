"""bench.py --dump-outputs on CPU: a proof struct packed from known values is written as
DIR/<name>.npy (float64, 16 limbs of 16 bits per field element) and read back exactly; the
options a plain and a --full run are told apart by are parsed."""
import os
import sys

import numpy as np

from oracle import pyoracle as po

import bench
import twist_and_shout as ts

R, P = ts.R_MOD, ts.P_MOD


def _ints(a):
    return [sum(int(x) << (16 * j) for j, x in enumerate(row)) for row in a.reshape(-1, 16)]


def test_limbs16_is_exact_at_the_field_edges():
    vals = [0, 1, 0xFFFF, 1 << 16, R - 1, P - 1, (1 << 256) - 1]
    a = bench._limbs16(vals)
    assert a.dtype == np.float64 and a.shape == (len(vals), 16)
    assert a.min() >= 0 and a.max() <= 0xFFFF
    assert _ints(a) == vals
    assert bench._limbs16([]).shape == (0, 16)


def test_dump_outputs_round_trips_a_packed_proof(tmp_path):
    pts = [po.G1_GEN, None, po.affine_mul(po.G1_GEN, R - 5), po.affine_mul(po.G1_GEN, 123456789)]
    rounds = [[(7 * r + c) * (R // 11) % R for c in range(4)] for r in range(5)]
    finals = [R - 1, 3]
    raw = ts._pack_proof(pts[:2], rounds, R - 2, pts[2:], finals)
    d = tmp_path / "dump"
    bench.dump_outputs(ts, raw, str(d))
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["commitments", "final_evaluation", "final_evaluations", "final_mle_evals",
                           "opening_point", "opening_proofs", "round_polynomials", "sumcheck_challenges"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) < 64 << 20
    assert got["commitments"].shape == (2, 2, 16) and got["round_polynomials"].shape == (5, 4, 16)
    flat = lambda ps: [c for Q in ps for c in (Q if Q is not None else (0, 0))]  # noqa: E731
    assert _ints(got["commitments"]) == flat(pts[:2])
    assert _ints(got["opening_proofs"]) == flat(pts[2:])
    assert _ints(got["round_polynomials"]) == [c for r in rounds for c in r]
    assert _ints(got["final_evaluation"]) == [R - 2]
    assert _ints(got["final_evaluations"]) == finals


def test_plain_and_full_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"
