"""CPU test of Loss.__call__ as the kernels evaluate it (ampligraph_amd/csrc/kge_loss.h: the one definition the forward kernel and the
column-sharded loss kernel share): the header compiled with g++ into a small harness (tests/csrc/loss_check.cpp) that runs the serial
walk -- one thread per positive, the walk of cols_loss_kernel.  Checked against oracle.kge_oracle.loss_and_grads (loss_functions.py:185-225
and the five _apply_loss bodies, fp64) to the tolerances tests/test_gpu_cols.py applies to the same quantities, and against the NaN / inf
rules the header's comments state."""
import os
import subprocess

import numpy as np
import pytest

from oracle import kge_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSSES = ["pairwise", "nll", "absolute_margin", "self_adversarial", "multiclass_nll"]   # index = AMDKGE_LOSS_*
NEG_ZERO = 0x80000000


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("loss") / "loss_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", "loss_check.cpp"), "-o", exe], check=True)
    return exe


def run(harness, loss, mean, P, N):
    """Loss.__call__ of the header for positives P [n] with corruption scores N [n][eta] -> per [n], dP [n], dN [n][eta] (fp32)."""
    prm = dict(O.LOSS_DEFAULTS[loss])
    head = f"{LOSSES.index(loss)} {prm.get('margin', 0.0)!r} {prm.get('alpha', 0.0)!r} {int(mean)} {N.shape[1]}"
    text = "".join(f"{head} {float(p).hex()} " + " ".join(float(v).hex() for v in row) + "\n" for p, row in zip(P, N))
    out = subprocess.run([harness], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(P)
    vals = np.array([[float.fromhex(t) for t in line.split()] for line in out], dtype=np.float32)
    return vals[:, 0], vals[:, 1], vals[:, 2:]


def drawn_scores(rng, eta, n=48):
    """Positives and corruption scores on both branches of the hinges (margin - P + n and margin + n of either sign) and on both sides
    of both ends of the [-75, 75] clip.  Rows 0..n/4: a positive above 75; n/4..n/2: a positive below -75 (their corruptions stay
    moderate: next to a corruption above 75 the multiclass term e^P / Z would leave fp32's range, where the fp64 oracle cannot
    follow); every other row has corruptions beyond both ends of the clip."""
    P = (rng.normal(size=n) * 3).astype(np.float32)
    N = (rng.normal(size=(n, eta)) * 3).astype(np.float32)
    q = n // 4
    P[:q] = rng.uniform(75.5, 120, q)
    P[q:2 * q] = -rng.uniform(75.5, 120, q)
    far = rng.random((n, eta)) < 0.3
    far[:, 0] = True                                  # (eta = 1 too)
    far[q:2 * q] = False
    hi = rng.random((n, eta)) < 0.5
    hi[2 * q:3 * q] &= rng.random((q, 1)) < 0.5       # some rows with nothing above 75, some with both ends
    N = np.where(far, np.where(hi, rng.uniform(75.5, 120, (n, eta)), -rng.uniform(75.5, 120, (n, eta))), N).astype(np.float32)
    N[0, 0], N[1, 0], P[2 * q] = 75.0, -75.0, 75.0    # the ends themselves are inside
    return P, N


@pytest.mark.parametrize("eta", [1, 7, 64, 65])
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("loss", LOSSES)
def test_serial_walk_against_oracle(harness, loss, mean, eta):
    rng = np.random.default_rng(1000 * LOSSES.index(loss) + 10 * eta + mean)
    P, N = drawn_scores(rng, eta)
    assert (N > 75).any() and (N < -75).any() and (P > 75).any() and (P < -75).any()
    m = O.LOSS_DEFAULTS[loss].get("margin", 1.0)
    for h in (m - P[:, None] + N, m + N):
        assert (h > 0).any() and (h < 0).any()
    per, dP, dN = run(harness, loss, mean, P, N)
    total, rper, rdP, rdN = O.loss_and_grads(loss, P, N.T.reshape(-1), eta, None, "mean" if mean else "sum")
    rdN = rdN.reshape(eta, -1).T
    assert np.all(np.abs(per - rper) <= 3e-5 * np.maximum(1.0, np.abs(rper))), np.abs(per - rper).max()
    tot = float(per.astype(np.float64).sum())
    assert abs(tot - float(total)) <= 3e-5 * max(1.0, abs(float(total))), (tot, float(total))
    scale = max(np.abs(rdN).max(), np.abs(rdP).max(), 1e-30)
    assert np.allclose(dP, rdP, rtol=2e-4, atol=2e-5 * scale), np.abs(dP - rdP).max()
    assert np.allclose(dN, rdN, rtol=2e-4, atol=2e-5 * scale), np.abs(dN - rdN).max()


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("loss", LOSSES)
def test_non_finite_rules(harness, loss, mean):
    """clip_exp / hinge_nan: a NaN score is a NaN loss value.  masked_zero: a coefficient that a clip or hinge mask sets to zero is +0.0
    for a finite score and -0.0 for a non-finite one.  computed_zero: the self-adversarial coefficient of a -inf score is -0.0."""
    nan, inf = np.float32("nan"), np.float32("inf")
    base = np.array([0.5, -1.0, 2.0, 0.25, -0.5], dtype=np.float32)
    bits = lambda a: np.asarray(a, dtype=np.float32).view(np.uint32)   # noqa: E731
    # a NaN positive, a NaN corruption (first, middle, last and only)
    rows = [(nan, base)] + [(0.3, np.where(np.arange(5) == j, nan, base)) for j in (0, 2, 4)]
    per, _, _ = run(harness, loss, mean, np.array([r[0] for r in rows], dtype=np.float32), np.stack([r[1] for r in rows]).astype(np.float32))
    assert np.isnan(per).all(), per
    per, _, _ = run(harness, loss, mean, np.array([0.3], dtype=np.float32), np.array([[nan]], dtype=np.float32))
    assert np.isnan(per).all(), per
    if loss == "self_adversarial":
        N = base.copy()
        N[3] = -inf
        _, _, dN = run(harness, loss, mean, np.array([0.3], dtype=np.float32), N[None])
        assert bits(dN[0, 3]) == NEG_ZERO and np.isfinite(dN[0]).all() and np.all(dN[0, [0, 1, 2, 4]] != 0), dN
        return
    # masked coefficients: a finite score outside the clip / on the inactive side of the hinge, then the non-finite ones
    clip = loss in ("nll", "multiclass_nll")
    finite = [80.0, -80.0] if clip else [-50.0]
    nonfinite = [inf, -inf, nan] if clip else [-inf, nan]   # (+inf is the ACTIVE side of a hinge: coefficient 1 / red)
    for vals, want in ((finite, 0), (nonfinite, NEG_ZERO)):
        for v in vals:
            N = base.copy()
            N[1] = v
            _, _, dN = run(harness, loss, mean, np.array([0.3], dtype=np.float32), N[None])
            assert bits(dN[0, 1]) == want, (v, dN)
