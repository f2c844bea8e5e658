"""amdkge_opt_step_rows on a table of more than 2^31 floats, in the manner of tests/test_gpu_wide_offsets.py: the narrow geometry of
tests/wide_tables.py (5 500 858 rows x 400 floats: row i = base[i % 4 099]), SGD so that only the table and its gradient are that
large.  The listed rows lie on both sides of element 2^31 -- the row that crosses it and the first row beyond it among them -- and
include the table's last row; they are held to the oracle's rule on their compact copy, and EVERY other row of the table and of the
gradient to its bits by the helpers' sampled comparison.  A row offset that wrapped at 32 bits would read another base row and dirty a
row the test holds to its bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import wide_tables as WT
from oracle import kge_oracle as O
from test_gpu_kernels import dev
from wide_tables import NARROW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def narrow(gpu_lib):
    yield NARROW
    WT.release_all()


def test_opt_step_rows_beyond_2_31_elements(gpu_lib, narrow):
    from ampligraph_amd import _ffi

    geo, lam, lr = narrow, 1e-3, 1e-2
    eng = geo.engine("DistMult", 400)
    geo.fill("gaussian")
    geo.training(eng, "sgd")
    assert eng.ent.numel() > 2 ** 31
    rng = np.random.default_rng(79)
    stray = np.array([geo.first_high + 2, geo.N - 3, 2])
    listed = np.setdiff1d(np.concatenate([geo.spread_ids(rng, 300), [0, 1, geo.first_high - 2, geo.first_high + 1, geo.N - 2]]), stray)
    assert listed[-1] == geo.N - 1 and (listed * geo.Ks < 2 ** 31).any() and (listed * geo.Ks > 2 ** 31).sum() > 100
    # gradient on two thirds of the listed rows -- and on three rows that are NOT listed: they keep everything, gradient included
    hot = listed[rng.random(listed.size) < 0.67]
    hot = np.union1d(hot, [geo.N - 1, geo.first_high, geo.first_high - 1])
    G = (rng.normal(size=(hot.size + stray.size, geo.Ks)) * 0.1).astype(np.float32)
    try:
        eng.g_ent[dev(np.concatenate([hot, stray]))] = dev(G)
        rows = dev(np.concatenate([listed, [5, 5, 5]]).astype(np.int32))     # behind the count: never read
        n_rows = dev(np.array([listed.size], np.int64))
        opt = _ffi.Opt(_ffi.OPTIMIZERS["sgd"], 2, lr, 0.9, 0.999, 1e-7, lam, 1, 0, geo.Ks)
        _ffi.check(eng.lib.amdkge_opt_step_rows(C.byref(opt), eng.ent.data_ptr(), eng.g_ent.data_ptr(), None, None, geo.N, rows.data_ptr(),
                                                n_rows.data_ptr(), int(rows.numel()), eng.loss_acc.data_ptr() + 8, None))
        torch.cuda.synchronize()
        x0 = geo.rows(hot)
        st = O.TrainState(x0, geo.rel, "sgd", lr)
        want_reg = O.apply_optimizer_lazy(st, G[:hot.size].astype(np.float64), np.zeros(geo.rel.shape), dict(p=2, lam_e=lam, lam_r=0.0))
        got = eng.ent[dev(hot)].cpu().numpy()
        # test_gpu_kernels::test_opt_step_parity's bars: 2e-6 on the parameters, 1e-5 on reg_loss
        assert np.abs(got - st.ent).max() <= 2e-6 * max(1.0, np.abs(st.ent).max()), np.abs(got - st.ent).max()
        assert np.abs(got - x0).max() > 1e-4
        assert abs(float(eng.loss_acc[1]) - want_reg) <= 1e-5 * want_reg, (float(eng.loss_acc[1]), want_reg)
        geo.assert_only(geo.rows_differing(), hot, "opt_step_rows: table")                       # every other row: its bits
        geo.assert_only(geo.rows_nonzero(eng.g_ent), stray, "opt_step_rows: gradient")            # reset on the listed rows, and only there
        assert np.array_equal(eng.g_ent[dev(stray)].cpu().numpy(), G[hot.size:])
    finally:
        geo.restore()
        eng.g_ent[dev(np.concatenate([hot, stray]))] = 0.0
