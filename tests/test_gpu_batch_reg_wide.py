"""amdkge_batch_reg_fwdbwd beyond 2^31 table elements, in the manner of tests/test_gpu_wide_offsets.py: the narrow geometry of
tests/wide_tables.py (5 500 858 rows x 400 floats, ComplEx k = 200: row i = base[i % 4 099]), positives whose entity rows lie in window
S -- straddling element offset 2^31 -- and in window T, the table's last rows.  The gradient of the window against the restatement on
the window's compact copy (the bars of tests/test_gpu_batch_reg.py), and over ALL rows of the gradient table: no row outside the touched
set holds a set bit.  An offset that wrapped at 32 bits would read another base row and dirty a row below the mark."""
import numpy as np
import pytest
import torch

import batch_reg_ref as BR
import wide_tables as WT
from test_gpu_kernels import dev
from wide_tables import M, NARROW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def narrow(gpu_lib):
    yield NARROW
    WT.release_all()


@pytest.mark.parametrize("window", ["S", "T"])
def test_batch_reg_beyond_2_31_elements(gpu_lib, narrow, window):
    from ampligraph_amd.latent_features.regularizers import BatchLPRegularizer

    geo, model, k = narrow, "ComplEx", 200
    lo = getattr(geo, window)
    eng = geo.engine(model, k)
    geo.fill("gaussian")
    geo.training(eng, "sgd")
    rng = np.random.default_rng(71)
    B = 257
    X, Xc = geo.window_triples(rng, lo, B)
    X[0, 0], Xc[0, 0] = lo + M - 1, M - 1                                   # the window's last row (T: the table's)
    if window == "S":
        X[1, 2], Xc[1, 2] = geo.first_high, geo.first_high - lo              # the first row that starts beyond element 2^31 - 1 ...
        X[2, 0], Xc[2, 0] = geo.first_high - 1, geo.first_high - 1 - lo      # ... and the row that crosses it
    reg_e, reg_r = BatchLPRegularizer(3, 0.05), BatchLPRegularizer(2, 0.125, "float")
    eng.batch_reg_fwdbwd(dev(X), reg_e, reg_r)
    torch.cuda.synchronize()
    R = float(eng.loss_acc[1].item())
    assert float(eng.loss_acc[0].item()) == 0.0
    wR, wGe, wGr = BR.batch_reg(model, k, geo.window(lo), geo.rel, Xc, 3, 0.05, BR.MODULUS, 2, 0.125, BR.FLOAT)
    assert abs(R - wR) <= 1e-6 * wR
    BR.assert_rows_close(eng.g_ent[lo:lo + M].cpu().numpy(), wGe, 1e-5)
    BR.assert_rows_close(eng.g_rel.cpu().numpy(), wGr, 1e-5)
    geo.assert_only(geo.rows_nonzero(eng.g_ent), np.concatenate([X[:, 0], X[:, 2]]), "batch_reg_fwdbwd")
    assert int(geo.rows_differing().sum().item()) == 0                       # the table itself is an input
    eng.g_flat.zero_()
