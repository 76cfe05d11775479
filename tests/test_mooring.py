"""Quasi-static mooring lines off the device: the longdouble reference and the fp64 model of the kernels against the
recorded tensions of the reference's decks, the YAML parser and its refusals, the sweep's mooring edits, and the gate
rejecting seeded errors (the kernels themselves: tests/test_hip_mooring.py)."""
import copy

import numpy as np
import pytest

from raft_amd import geometry, mooring
from raft_amd.strips import UnsupportedFOWT

from . import mooring_cases as mc
from . import mooring_device_model as dm
from . import mooring_reference as mr

# The reference's own tolerance on Tmoor_avg (its tests/test_model.py:366).  Measured with mooring_reference.py at the
# recorded mean poses (scripts/make_mooring_golden.py): VolturnUS-S 4.30e-08, VolturnUS-S-pointInertia 4.27e-08,
# OC3spar 5.86e-07, OC4semi-WAMIT_Coefs 7.09e-09.
TMOOR_RTOL = 1e-5


@pytest.mark.parametrize("deck", mc.DECKS)
def test_reference_and_model_reproduce_recorded_tensions(deck):
    g = mc.golden()[deck]
    lines = np.broadcast_to(g["lines"], (len(g["poses"]),) + g["lines"].shape)
    for ev in (mr.evaluate, dm.evaluate):
        res = ev(lines, g["poses"], g["depth"])
        assert not res["flags"].any()
        rel = np.abs(np.asarray(res["T"], dtype=float) - g["Tmoor_avg"]) / np.abs(g["Tmoor_avg"])
        print("%s %s: worst |T - Tmoor_avg| / Tmoor_avg = %.3g" % (deck, ev.__module__, rel.max()))
        assert rel.max() <= TMOOR_RTOL


def test_oc3spar_has_a_line_off_the_seabed():
    g = mc.golden()["OC3spar"]
    ref = mr.evaluate(np.broadcast_to(g["lines"], (len(g["poses"]),) + g["lines"].shape), g["poses"], g["depth"])
    assert set(ref["line_out"][..., 6].astype(int).ravel()) == {0, 1}


def test_model_within_gate():
    worst = 0.0
    for name, lines, pose, depth in mc.batches():
        ref = mc.reference()[name]
        res = dm.evaluate(lines, pose, depth)
        assert np.array_equal(res["flags"], ref["flags"]) and not ref["flags"].any(), name
        assert np.array_equal(res["line_out"][..., 6], ref["line_out"][..., 6].astype(float)), name      # the branch
        w = mc.worst_multiples(res, ref)
        print("%-36s kappa %.3g  %s" % (name, ref["kappa"].max(), w))
        worst = max(worst, max(w.values()))
    print("worst multiple of eps Ek: %.3g (recorded %.3g, gate %d)" % (worst, mr.GATE_WORST_CPU, mr.GATE_C))
    assert worst <= mr.GATE_C
    assert mr.GATE_C >= 4 * mr.GATE_WORST_CPU and mr.GATE_C & (mr.GATE_C - 1) == 0


def test_cases_cover_the_branches():
    ref = mc.reference()
    lo = lambda n: ref[n]["line_out"]
    assert np.all(lo("contact")[..., 6] == 1) and np.all(lo("contact")[..., 4] > 0)
    assert np.all(lo("anchor_off_seabed")[..., 6] == 0) and np.all(lo("anchor_off_seabed")[..., 3] < 0)
    assert np.all(lo("nearly_taut")[..., 6] == 0)
    rec, _ = mc.single_lines()["boundary_above"]
    wL = rec[8] * rec[6]
    a, b = lo("boundary_above")[0, 0], lo("boundary_below")[0, 0]
    assert a[6] == 0 and 0 < float(a[1] / wL - 1) < 2e-9
    assert b[6] == 1 and 0 < float(1 - b[1] / wL) < 2e-9


# (not the two boundary lines: the second derivative jumps between the branches, and a difference quotient across the
# jump is only O(h) accurate)
@pytest.mark.parametrize("name", ["contact", "no_contact", "anchor_off_seabed", "nearly_taut", "EA_1e6", "OC3spar"])
def test_reference_derivatives_against_central_differences(name):
    _, lines, pose, depth = [b for b in mc.batches() if b[0] == name][0]
    eC, eJ = mr.fd_check(lines[-1], pose[-1], depth)
    print("%s: analytic vs central differences, worst / envelope: C %.3g, J %.3g" % (name, eC, eJ))
    assert eC < 1e-6 and eJ < 1e-6        # h = 1e-4 m / rad: the differences' own O(h^2) error; a wrong term is O(1)


def test_flags_of_reference_and_model():
    rec, depth = mc.single_lines()["contact"]
    bad = {1: [(6, 0.0), (7, -1.0), (8, np.nan), (2, -201.0), (5, -205.0)], 2: [(0, -58.0)], 4: [(6, 2000.0)]}
    for flag, edits in bad.items():
        for i, v in edits:
            r = rec.copy()
            r[i] = v
            if flag == 2:
                r[6] = 400.0
            lines = np.stack([rec, r, rec])[:, None, :]
            for ev in (mr.evaluate, dm.evaluate):
                res = ev(lines, None, depth)
                assert list(res["flags"]) == [0, flag, 0], (flag, i, v)
                assert np.all(np.isnan(np.asarray(res["C"][1], dtype=float))) and np.all(np.isfinite(np.asarray(res["C"][[0, 2]], dtype=float)))


# ---------------------------------------------------------------------------------------------- parser
@pytest.mark.parametrize("deck", mc.DECKS)
def test_parser_on_the_decks(deck):
    g = mc.golden()[deck]
    lines, depth = mooring.lines_from_design(g["design"], rho=g["rho"], g=g["g"])
    assert depth == g["depth"] and np.array_equal(lines, g["lines"])
    moor = g["design"]["mooring"]
    lt = moor["line_types"][0]
    assert np.isclose(lines[0, 8], (lt["mass_density"] - g["rho"] * np.pi / 4 * lt["diameter"] ** 2) * g["g"], rtol=1e-14, atol=0)
    assert lines[0, 7] == float(lt["stiffness"]) and lines[0, 6] == float(moor["lines"][0]["length"])
    assert np.all(lines[:, 9:] == 0)


def test_parser_refusals():
    base = mc.golden()["VolturnUS-S"]["design"]

    def refused(edit, match):
        d = copy.deepcopy(base)
        edit(d["mooring"])
        with pytest.raises(UnsupportedFOWT, match=match):
            mooring.lines_from_design(d)

    refused(lambda m: m["points"][3].update(type="free"), "free points")
    refused(lambda m: m["lines"][0].update(endA="line2_vessel"), "both ends on the vessel")
    refused(lambda m: m["lines"][1].update(endA="line1_anchor"), "joins 2 lines")
    refused(lambda m: m.update(file="mooring.dat"), "MoorDyn file")
    refused(lambda m: m.update(moorMod=1), "moorMod")
    refused(lambda m: m["lines"][0].update(endA="line1_vessel", endB="line1_anchor"), "fixed point")
    with pytest.raises(UnsupportedFOWT):
        mooring.lines_from_design({"site": {}})


def test_tension_names():
    assert mooring.tension_names(2) == ["Tmoor_A1", "Tmoor_A2", "Tmoor_B1", "Tmoor_B2"]


# ---------------------------------------------------------------------------------------------- the sweep's edits
def test_volturnus_mooring_program_follows_the_columns():
    base = mc.golden()["VolturnUS-S"]["design"]
    P = geometry.volturnus_mooring_program(base)
    rng = np.random.default_rng(5)
    scales = np.concatenate([np.ones((1, 5)), np.full((1, 5), 0.75), np.full((1, 5), 1.25), rng.uniform(0.75, 1.25, (29, 5))])
    params = geometry.volturnus_params(scales)
    out = P.expand(params)
    ocD, ocR = params[:, 1], params[:, 3]
    rad = ocR + ocD / 2                                        # raft/parametersweep.py:79-83
    want = np.broadcast_to(P.lines, out.shape).copy()
    want[:, 0, 3] = -ocR - ocD / 2
    for l, deg in ((1, 60), (2, 300)):
        want[:, l, 3] = rad * np.cos(np.deg2rad(deg))
        want[:, l, 4] = rad * np.sin(np.deg2rad(deg))
    # the program adds c_ocD ocD + c_ocR ocR where the script multiplies the sum: two roundings apart at most
    assert np.allclose(out, want, rtol=4 * np.finfo(float).eps, atol=0)
    assert np.array_equal(out[..., [0, 1, 2, 5, 6, 7, 8]], want[..., [0, 1, 2, 5, 6, 7, 8]])
    assert np.array_equal(out[0, :, 3:5], np.array([[-58.0, 0.0], [58.0 * np.cos(np.deg2rad(60)), 58.0 * np.sin(np.deg2rad(60))],
                                                    [58.0 * np.cos(np.deg2rad(300)), 58.0 * np.sin(np.deg2rad(300))]]))
    ref = mr.evaluate(out[:3], None, 200.0)
    assert not ref["flags"].any()


# ---------------------------------------------------------------------------------------------- seeded errors
SEED_CASES = {"no_stretch": ("contact", "no_contact", "EA_1e6"), "lb_stretched": ("contact", "EA_1e6", "VolturnUS-S"),
              "arm_sign": ("contact", "OC3spar"), "no_coupling": ("contact", "OC3spar"), "ja_from_b": ("contact", "OC3spar")}


@pytest.mark.parametrize("seed", dm.SEEDS)
def test_gate_rejects_seeded_errors(seed):
    for name in SEED_CASES[seed]:
        _, lines, pose, depth = [b for b in mc.batches() if b[0] == name][0]
        w = mc.worst_multiples(dm.evaluate(lines, pose, depth, seed=seed), mc.reference()[name])
        print("%s on %s: %s" % (seed, name, w))
        assert max(w.values()) > mr.GATE_C
