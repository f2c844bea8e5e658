"""amdkge_train_relation_fwdbwd beyond 2^31 table elements, in the manner of tests/test_gpu_batch_reg_wide.py: the narrow geometry of
tests/wide_tables.py (5 500 858 rows x 400 floats, ComplEx k = 200: row i = base[i % 4 099]), positives whose entity rows lie in window
S, straddling element offset 2^31.  Scores, loss and the gradient of the window against the restatement on the window's compact copy
(the bars of tests/test_gpu_relation_objective.py), and over ALL rows of the gradient table: no row outside the touched set holds a
set bit.  An s / o row offset that wrapped at 32 bits would read another base row -- other scores -- and dirty a row below the mark."""
import numpy as np
import pytest
import torch

import relation_objective_ref as RR
import wide_tables as WT
from test_gpu_kernels import assert_grads_close, dev, loss_desc
from wide_tables import M, NARROW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def narrow(gpu_lib):
    yield NARROW
    WT.release_all()


def test_relation_objective_beyond_2_31_elements(gpu_lib, narrow):
    geo, model, k, lo = narrow, "ComplEx", 200, narrow.S
    eng = geo.engine(model, k)
    geo.fill("gaussian")
    geo.training(eng, "sgd")
    rng = np.random.default_rng(73)
    B, R, w = 257, geo.R, 0.25
    X, Xc = geo.window_triples(rng, lo, B)
    X[0, 0], Xc[0, 0] = lo + M - 1, M - 1                                   # the window's last row
    X[1, 2], Xc[1, 2] = geo.first_high, geo.first_high - lo                  # the first row that starts beyond element 2^31 - 1 ...
    X[2, 0], Xc[2, 0] = geo.first_high - 1, geo.first_high - 1 - lo          # ... and the row that crosses it
    known = [np.unique(np.array([p, (7 * i + 3) % R], dtype=np.int32)) for i, p in enumerate(X[:, 1])]
    mask, masked, unmaskable = RR.mask_matrix(B, R, known)
    ps = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    ns = torch.full((B * R,), 7.0, dtype=torch.float32, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    eng.train_relation_fwdbwd(dev(X), loss_desc("multiclass_nll"), w, flt=tuple(dev(a) for a in RR.csr(known)), stats=stats, pos_scores=ps, rel_scores=ns)
    torch.cuda.synchronize()
    L = float(eng.loss_acc[0].item())
    want, Te, Tr, sp, sn = RR.relation_step(model, geo.window(lo), geo.rel, Xc, mask, "multiclass_nll", "sum", w)
    live = np.isfinite(sn)
    got_ns, got_ps = ns.cpu().numpy(), ps.cpu().numpy()
    assert stats.cpu().tolist() == [masked, unmaskable] and np.array_equal(np.isneginf(got_ns), ~live)
    assert np.allclose(got_ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
    assert np.allclose(got_ns[live], sn[live], rtol=1e-5, atol=1e-5 * np.abs(sn[live]).max())
    assert abs(L - want) <= 1e-5 * max(1.0, abs(L)), (L, want)
    assert_grads_close(eng.g_ent[lo:lo + M].cpu().numpy().astype(np.float64), Te)
    assert_grads_close(eng.g_rel.cpu().numpy().astype(np.float64), Tr)
    geo.assert_only(geo.rows_nonzero(eng.g_ent), np.concatenate([X[:, 0], X[:, 2]]), "train_relation_fwdbwd")
    assert int(geo.rows_differing().sum().item()) == 0                       # the table itself is an input
    eng.g_flat.zero_()
