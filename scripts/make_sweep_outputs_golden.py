"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/refgold_sweep_outputs.npz from the LIVE reference (imported unmodified
through oracle/ref_harness.py, read-only).  Run in the build container only:

    python scripts/make_sweep_outputs_golden.py

Never imported by the tests; they read the committed .npz, which holds data only:

  * "ref": for four VolturnUS-S platform variants (oracle/make_golden.py volturnus_variant; the two scale rows of
    tests/test_dropin_live_reference.py test_member_description_sweep_equals_reference_models and two more) at
    min_freq = 0.01, max_freq = 0.3 (nw = 30) and two load cases -- one wave train, and two wave trains of different
    headings -- the reference's own Model -> solveDynamics -> FOWT.saveTurbineOutputs values of surge .. yaw_std,
    AxRNA / AyRNA / AzRNA_std and Mbase_std, [variant, case(, rotor)];
  * "sweep": everything GeometrySweep(...) needs to solve the same variants for the same sea states -- the member
    descriptions, M_extra / B0 / C_extra of raft_amd.dropin.sweep_from_member_tables, the frequency axis, zeta / beta with
    the one-train case padded by a second train of zero amplitude;
  * "rows": raft_amd.dropin.sweep_output_rows of the base unit (shared by the variants: one turbine, no line system).

Before writing, the script solves the fixture on the CPU oracle's resident path (sweep.upload, run_channels) and holds the
result to the gate the tests use -- 1e-8 x the key's largest value + 1e-12, as tests/test_dropin_live_reference.py does for
these keys: a miss is a finding about the feeder, not a reason to widen the gate.
"""
import contextlib
import copy
import io
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh          # noqa: E402
from oracle import make_golden as mg          # noqa: E402
from raft_amd import snapshot as standin      # noqa: E402
from raft_amd import dropin, geometry as G    # noqa: E402
from raft_amd._abi import RaftxLib            # noqa: E402

OUT = os.path.join(standin.GOLDEN_DIR, "refgold_sweep_outputs.npz")
SETTINGS = dict(min_freq=0.01, max_freq=0.3)
SCALES = np.array([[1.1, 0.9, 1.05, 0.95, 1.2], [0.8, 1.2, 0.9, 1.1, 0.85],          # tests/test_dropin_live_reference.py:129
                   [1.0, 1.0, 1.0, 1.0, 1.0], [0.9, 1.1, 1.15, 0.85, 1.05]])
MOTIONS = ("surge", "sway", "heave", "roll", "pitch", "yaw")
KEYS = tuple(m + "_std" for m in MOTIONS) + ("AxRNA_std", "AyRNA_std", "AzRNA_std", "Mbase_std")
DEG = 57.29577951308232                       # helpers.rad2deg


def load_cases():
    one = rh.make_case(Hs=4.0, Tp=9.0, heading=20.0)
    two = rh.make_case(Hs=4.0, Tp=9.0, heading=20.0)
    two.update(wave_heading=[20.0, -60.0], wave_spectrum=["JONSWAP", "JONSWAP"], wave_period=[9.0, 13.0],
               wave_height=[4.0, 2.0], wave_gamma=[0, 0])
    return [one, two]


def gate_miss(got, ref):
    """Largest |got - ref| / (1e-8 max|ref| + 1e-12) of one key's values."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    return float(np.max(np.abs(got - ref)) / (1e-8 * np.max(np.abs(ref)) + 1e-12))


def full_rows(L, Gw, nw):
    """The six motions (rotations in degrees) in front of the output rows: the channel set of saveTurbineOutputs."""
    Lf = np.zeros((6 + len(L), 3, 6))
    for j in range(6):
        Lf[j, 0, j] = 1.0 if j < 3 else DEG
    Lf[6:] = L
    Gf = None
    if Gw is not None:
        Gf = np.zeros((len(Lf), 6, nw), dtype=complex)
        Gf[6:] = Gw
    return Lf, Gf


def main():
    rh.import_raft()
    from raft_amd import waves
    base = rh.prepare_design(rh.load_design(os.path.join(rh.REFERENCE_ROOT, "examples/VolturnUS-S_example.yaml")), settings=SETTINGS)
    cases = load_cases()
    designs = [mg.volturnus_variant(base, s) for s in SCALES]
    nD, nC = len(designs), len(cases)
    ref = {}
    with contextlib.redirect_stdout(io.StringIO()):
        m0 = rh.build_model(copy.deepcopy(base))
        for d, design in enumerate(designs):
            for c, case in enumerate(cases):
                m = rh.build_model(copy.deepcopy(design))
                m.solveDynamics(copy.deepcopy(case))
                res = {}
                m.fowtList[0].saveTurbineOutputs(res, copy.deepcopy(case))
                for key in KEYS:
                    v = np.atleast_1d(np.asarray(res[key], dtype=float))
                    ref.setdefault(key, np.zeros((nD, nC) + v.shape))[d, c] = v
    f0 = m0.fowtList[0]
    nw = int(m0.nw)
    # the sweep: member descriptions of the variants, the base model's non-geometry terms
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)
    ctx = RaftxLib(os.path.join(ROOT, "oracle", "libraftx_oracle.so")).context(0)
    tabs = G.concat_units([G.describe_unit(d) for d in designs])
    sweep = dropin.sweep_from_member_tables(m0, G.describe_unit(base), tabs, [cases[0]], ctx)
    zeta, beta = np.zeros((nC, 2, nw)), np.zeros((nC, 2))
    for c, case in enumerate(cases):
        n, b, _, z = waves.sea_state(copy.deepcopy(case), f0.w, f0.dw)
        zeta[c, :n], beta[c, :n] = z, b
    sweep.zeta, sweep.beta = np.ascontiguousarray(zeta), np.ascontiguousarray(beta)
    names, L, Gw = dropin.sweep_output_rows(f0)
    assert names == ["AxRNA[0]", "AyRNA[0]", "AzRNA[0]", "Mbase[0]"], names
    # the check: the oracle's resident path on exactly what is written below
    Lf, Gf = full_rows(L, Gw, nw)
    sweep.upload(ctx)
    got = sweep.run_channels(ctx, Lf, Gw=Gf)
    assert np.all(got["flags"] & 1) and not np.any(got["flags"] & 2), got["flags"]
    worst = 0.0
    for i, key in enumerate(KEYS):
        for d in range(nD):
            for c in range(nC):
                miss = gate_miss(got["std"][d, c, i], ref[key][d, c])
                worst = max(worst, miss)
                assert miss <= 1.0, (key, d, c, miss, got["std"][d, c, i], ref[key][d, c])
    print("oracle resident path against the reference: worst %.3g of the gate 1e-8 max + 1e-12" % worst)
    ctx.close()
    t = sweep.tables
    fx = {"config": "reference saveTurbineOutputs standard deviations of four VolturnUS-S variants x two load cases (nw = 30), "
                    "the GeometrySweep inputs of the same variants and the output rows of the base unit",
          "scales": SCALES, "keys": list(KEYS), "ref": ref,
          "sweep": {"member_off": np.asarray(t.member_off), "members": np.asarray(t.members), "station_off": np.asarray(t.station_off),
                    "stations": np.asarray(t.stations), "cap_off": np.asarray(t.cap_off), "caps": np.asarray(t.caps),
                    "M_extra": sweep.M0, "B0": sweep.B0, "C_extra": sweep.C0, "w": sweep.w, "k": sweep.k, "depth": sweep.depth,
                    "zeta": sweep.zeta, "beta": sweep.beta, "nIter": sweep.nIter, "XiStart": sweep.XiStart, "tol": sweep.tol,
                    "add_mask": sweep.add_mask, "rho": sweep.rho, "g": sweep.g},
          "rows": {"names": names, "L": L, "Gw": Gw}}
    assert sweep.pose is None and sweep.MBw is None
    standin.save_fixture(OUT, fx)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
