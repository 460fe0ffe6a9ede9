"""CPU: the float64 restatement of the masked losses (tests/loss_ref.py) against the real reference's fixtures (g9: realistic
inputs; g14: the edges, oracle/gen_golden_losses.py) and against the reference algorithm run with torch fp32 ops, plus the
host-side checks of deepblast_amd.losses that need no device."""
import os

import numpy as np
import pytest
import torch

import loss_ref

FIRST = {"mce": "Yt", "path": "P", "align": "Yt"}


def _close(got, ref, rel):
    """Values: NaN must match NaN, else |got - ref| <= rel * max(1, |ref|)."""
    if np.isnan(ref):
        return np.isnan(got)
    return abs(got - ref) <= rel * max(1.0, abs(ref))


def _grad_close(got, ref, rel):
    return np.max(np.abs(got - ref)) <= rel * max(1.0, float(np.abs(ref).max()))


def _g14_cases(d):
    return sorted({k.split("_")[0] for k in d.files})


@pytest.mark.parametrize("name", loss_ref.NAMES)
def test_restatement_reproduces_g9(golden_dir, name):
    d = np.load(os.path.join(golden_dir, "g9_losses.npz"))
    lens = d["lens"]
    r = loss_ref.loss(name, d[FIRST[name]], d["Yp"], lens[:, 0], lens[:, 1], d["G"])
    assert _close(r["loss"], float(d[name + "_loss"]), 1e-6)
    assert _grad_close(r["grad"], d[name + "_grad"], 1e-6)


@pytest.mark.parametrize("name", loss_ref.NAMES)
def test_restatement_reproduces_g14_edges(golden_dir, name):
    d = np.load(os.path.join(golden_dir, "g14_losses_edges.npz"))
    cases = _g14_cases(d)
    assert cases == ["c13", "c14", "c15", "c16", "e"]
    for case in cases:
        lens = d[case + "_lens"]
        r = loss_ref.loss(name, d[f"{case}_{FIRST[name]}"], d[case + "_Yp"], lens[:, 0], lens[:, 1], d[case + "_G"])
        ref, gref = float(d[f"{case}_{name}_loss"]), d[f"{case}_{name}_grad"]
        assert _close(r["loss"], ref, 1e-6), (case, r["loss"], ref)
        assert _grad_close(r["grad"], gref, 1e-6), (case, np.max(np.abs(r["grad"] - gref)))
        # exactly zero where the reference's gradient is: outside G, outside the block, behind the clamp
        assert not r["grad"][gref == 0].any(), case
        assert (r["grad"] != 0).sum() == (gref != 0).sum(), case


def test_g14_covers_the_edges(golden_dir):
    """The fixture holds what it claims to (so that a regenerated one cannot quietly lose an edge)."""
    d = np.load(os.path.join(golden_dir, "g14_losses_edges.npz"))
    assert {d[c + "_Yp"].shape[2] % 4 for c in ("c13", "c14", "c15")} == {1, 2, 3}
    yp = np.concatenate([d[c + "_Yp"].ravel() for c in _g14_cases(d)])
    lo, hi = loss_ref.EPS_LO, loss_ref.EPS_HI
    for v in (lo, np.nextafter(lo, np.float32(0)), np.nextafter(lo, np.float32(1)), hi, np.nextafter(hi, np.float32(0)),
              np.nextafter(hi, np.float32(2)), 0.0, 1.0):
        assert (yp == v).any(), v
    assert (yp < 0).any() and (yp > 1).any()
    g = np.concatenate([d[c + "_G"].ravel() for c in _g14_cases(d)])
    assert np.isnan(g).any() and (g == 0.5).any() and (g == -1).any()
    yt = d["c13_Yt"]
    assert ((yt > 0) & (yt < 1)).any()
    lens = d["e_lens"]
    assert (lens == 0).any() and (lens[:, 0] > 5).any() and np.isnan(d["e_mce_loss"])
    assert (d["c13_lens"][1] > d["c13_Yp"].shape[1:]).all()
    assert 0 < np.abs(d["c13_Yp"][3]).max() < 1e-19 and not d["c14_Yp"][4].any()


def _torch_edges(seed, B, N, M):
    c = loss_ref.edge_case(seed, B, N, M)
    c["lens"][0] = (N, M)
    c["lens"][-1] = (N + 2, M + 3)
    return c


@pytest.mark.parametrize("M", [1, 2, 3, 5, 13, 16])
@pytest.mark.parametrize("name", loss_ref.NAMES)
def test_restatement_matches_torch_fp32_at_the_edges(name, M):
    B, N = 5, 7
    c = _torch_edges(500 + M, B, N, M)
    if M >= 5:
        c["Yp"][1] = (1e-20 * np.random.default_rng(M).uniform(0.5, 2.0, (N, M))).astype(np.float32)   # tiny vectors
        c["Yt"][1] = 0.0
        c["P"][1] = 1.0
        c["Yp"][2] = c["Yt"][2] = 0.0                                                                     # a zero vector
    lens = c["lens"]
    xl, yl = lens[:, 0].tolist(), lens[:, 1].tolist()
    for empty in (False, True):
        G = c["G"].copy()
        if empty:
            G[3] = 0.0          # mean([]) = NaN
        yp = torch.tensor(c["Yp"], requires_grad=True)
        t = loss_ref.torch_reference(name, torch.tensor(c[FIRST[name]]), yp, xl, yl, torch.tensor(G))
        t.backward()
        r = loss_ref.loss(name, c[FIRST[name]], c["Yp"], xl, yl, G)
        assert _close(r["loss"], float(t.detach()), 1e-6), (r["loss"], float(t.detach()))
        gref = yp.grad.numpy()
        assert _grad_close(r["grad"], gref, 1e-6)
        assert not r["grad"][gref == 0].any() and not gref[r["grad"] == 0].any()
        if empty and name == "mce":
            assert np.isnan(r["loss"])


def test_restatement_clamp_is_inclusive_at_both_bounds():
    lo, hi = loss_ref.EPS_LO, loss_ref.EPS_HI
    assert lo == np.float32(3e-8) and hi == np.float32(0.99999994)
    Yp = np.array([[[lo, np.nextafter(lo, np.float32(0)), hi, np.nextafter(hi, np.float32(2))]]], np.float32)
    r = loss_ref.loss("mce", np.full_like(Yp, 0.5), Yp, [1], [4], np.ones_like(Yp))
    assert r["grad"][0, 0, 0] != 0 and r["grad"][0, 0, 1] == 0 and r["grad"][0, 0, 2] != 0 and r["grad"][0, 0, 3] == 0


@pytest.mark.parametrize("bad", [([-1, 3], [4, 4]), ([2, 3], [4, -2])])
def test_negative_loss_lengths_are_refused(bad):
    """The reference's slice [:-k] keeps all rows but the last k; the kernels would count nothing.  Neither is meant."""
    from deepblast_amd import losses
    with pytest.raises(ValueError, match="negative"):
        losses._lens(bad[0], bad[1], 2, "cpu")
    assert losses._lens([0, 3], [4, 0], 2, "cpu").tolist() == [[0, 4], [3, 0]]
