"""CPU-side checks of the drop-in surface: registries, defaults and error behaviour mirror the reference
(loss_functions.py:720-766, optimizers.py:255-291, regularizers.py:40-73), and the C-ABI library loads
and exports every symbol include/amdkge.h declares (no compute without a GPU)."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    """lib() raises unless the library exports every entry of _ffi.ABI, which tests/test_abi_host.py holds equal to the headers"""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    assert lib.amdkge_abi_version() == 5 == _ffi.ABI_VERSION
    assert lib.amdkge_internal_k(2, 200) == 400 and lib.amdkge_internal_k(0, 50) == 50


def test_abi_argument_validation_without_gpu():
    """Error paths that return before touching the device work on a GPU-less box."""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    m = _ffi.Model(9, 10, 5, 5, 0, 0)
    assert lib.amdkge_score(ctypes.byref(m), None, None, None, 1, None, None) == -1
    assert b"scoring_type" in lib.amdkge_last_error()
    m = _ffi.Model(2, 10, 5, 5, 0, 0)
    assert lib.amdkge_score(ctypes.byref(m), None, None, None, 0, None, None) == 0       # empty input is a no-op
    assert lib.amdkge_score(ctypes.byref(m), None, None, None, 3, None, None) == -1      # NULL pointers
    assert lib.amdkge_rank_compose(None, None, 3, 7, None, 1, None) == -1                # unknown strategy
    assert lib.amdkge_filter_ranges(None, None, 0, None, 5, 3, 10, 2, None, None, None) == -1   # bad side
    assert lib.amdkge_filter_ranges(None, None, 0, None, 0, 1, 10, 2, None, None, None) == 0    # empty batch
    import ctypes as C
    assert lib.amdkge_session_create(None, None) == -1
    bad = _ffi.SessionConfig()                                                                   # zeroed: k = 0
    h = C.c_void_p()
    assert lib.amdkge_session_create(C.byref(bad), C.byref(h)) == -1 and not h.value
    assert lib.amdkge_session_train_step(None, None, 3, None, None) == -1
    assert lib.amdkge_session_rank(None, None, 3, None, None, None, None, None, 0, 3, 0, None) == -1
    lib.amdkge_session_destroy(None)                                                             # no-op
    o = _ffi.Opt(2, 2, 1e-3, 0.9, 0.999, 1e-7, 0.0, 0)
    assert lib.amdkge_opt_step(ctypes.byref(o), None, None, None, None, 0, None, None) == -1   # iteration is 1-based
    o = _ffi.Opt(2, 2, 1e-3, 0.9, 0.999, 1e-7, 0.0, 1)
    assert lib.amdkge_opt_step(ctypes.byref(o), None, None, None, None, 0, None, None) == 0
    assert lib.amdkge_train_tiled_workspace_bytes(ctypes.byref(m), 100, 5) == 0                 # dense rows with k % 4 != 0
    mp = _ffi.Model(2, 10, 5, 5, 0, lib.amdkge_padded_k(10))                                    # ... padded to 12: supported
    assert lib.amdkge_padded_k(10) == 12 and lib.amdkge_row_floats(ctypes.byref(mp)) == 24
    assert lib.amdkge_train_tiled_workspace_bytes(ctypes.byref(mp), 100, 5) > 0
    assert lib.amdkge_row_floats(ctypes.byref(_ffi.Model(2, 10, 5, 5, 0, 8))) == -1              # k_pad < k
    assert lib.amdkge_pack_rows(ctypes.byref(mp), None, 0, None, None) == 0 and lib.amdkge_pack_rows(ctypes.byref(mp), None, 2, None, None) == -1
    assert lib.amdkge_set_rank_kernel(4) == -1 and lib.amdkge_set_rank_kernel(3) == 0 and lib.amdkge_set_rank_kernel(0) == 0
    m4 = _ffi.Model(2, 200, 14505, 237, 0, 0)
    assert lib.amdkge_train_tiled_workspace_bytes(ctypes.byref(m4), 10000, 20) > 10000 * 4 * 400 * 4
    assert lib.amdkge_train_step_tiled(ctypes.byref(m4), None, ctypes.byref(o), *([None] * 6), 0.0, None, 1, 1, 0, 1,
                                       0, 0, 0, 0, None, None, None, 1, 0, *([None] * 6)) == -1
    assert lib.amdkge_internal_k(7, 3) == -1


def test_registries_and_defaults():
    from ampligraph_amd.latent_features import loss_functions as lf
    from ampligraph_amd.latent_features import optimizers, regularizers

    assert set(lf.LOSS_REGISTRY) == {"pairwise", "nll", "absolute_margin", "self_adversarial", "multiclass_nll"}
    assert lf.get("pairwise")._loss_parameters == {"reduction": "sum", "margin": 1}
    sa = lf.get("self_adversarial")
    assert sa._loss_parameters["margin"] == 3 and sa._loss_parameters["alpha"] == 0.5
    assert lf.get("nll", {"reduction": "mean"}).to_ffi().reduction_mean == 1
    with pytest.raises(ValueError):
        lf.get("hinge")
    with pytest.raises(AssertionError):
        lf.get("nll", {"reduction": "median"})
    with pytest.raises(NotImplementedError):
        lf.get(lambda p, n: p)
    o = optimizers.get("adam")
    assert o.learning_rate == 0.001 and o.epsilon == 1e-7 and o.beta_1 == 0.9      # optimizers.py:284
    assert optimizers.get("adam", {"learning_rate": 5e-3}).learning_rate == 5e-3
    with pytest.raises(ValueError):
        optimizers.get("lion")
    with pytest.raises(ValueError):
        optimizers.get(3.0)
    r = regularizers.get("LP")
    assert (r.p, r.lam) == (2, 1e-5)
    assert regularizers.get("l3", {"lambda": 1e-3}).p == 3
    assert regularizers.get(None) is None
    with pytest.raises(ValueError):
        regularizers.get("elastic")


def test_model_surface_without_gpu():
    import numpy as np

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    with pytest.raises(KeyError):
        ScoringBasedEmbeddingModel(eta=1, k=2, scoring_type="ConvE")
    m = ScoringBasedEmbeddingModel(eta=5, k=10, scoring_type="RotatE")
    assert m.internal_k == 20 and not m.is_fit()
    with pytest.raises(AssertionError):   # RotatE forces GlorotUniform for relations (:1312-1315)
        m.compile(optimizer="adam", loss="nll", entity_relation_initializer=["glorot_uniform", "random_normal"])
    with pytest.raises(ValueError):
        m.compile(optimizer="adam", loss="not-a-loss")
    m.compile(optimizer="adam", loss="self_adversarial")
    with pytest.raises(AssertionError):
        m.get_count("e")
    with pytest.raises(RuntimeError):
        m.predict_proba(np.zeros((1, 3)))
    with pytest.raises(NotImplementedError):
        m.fit(np.array([["a", "b", "c"]]), partitioning_k=3)
    with pytest.raises(RuntimeError):     # fit before compile (:713)
        ScoringBasedEmbeddingModel(eta=1, k=2).fit(np.array([["a", "b", "c"]]))
    with pytest.raises(NotImplementedError):   # a Python callable cannot be fused into the HIP kernel: refused, not run on the host
        m.compile(optimizer="adam", loss=lambda pos, neg: pos)
    with pytest.raises(ValueError):       # optimizers.py:289
        m.compile(optimizer="not-an-optimizer", loss="nll")
    m.compile(optimizer="adam", loss="self_adversarial")
    with pytest.raises(AssertionError):   # :1605-1615
        m.evaluate(np.array([["a", "b", "c"]]), corrupt_side="x")
    twin = ScoringBasedEmbeddingModel.from_config(m.get_config())
    assert twin.get_config() == m.get_config() and twin.scoring_type == "RotatE"
    import torch

    if not torch.cuda.is_available():     # no GPU, no training: loudly, never a host fallback
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            m.fit(np.array([["a", "b", "c"], ["c", "b", "a"]]), batch_size=2, epochs=1)


def test_product_has_no_oracle_or_cpu_fallback():
    """The product package must never import the oracle (parity would be void)."""
    pkg = os.path.join(ROOT, "ampligraph_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(d, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


def test_compat_argument_mapping_and_session_without_gpu():
    """1.x adapter: argument mapping that needs no engine; the session layer fails loudly (error code + message, no crash,
    no fallback) when there is no GPU to create it on."""
    import torch

    from ampligraph_amd import _ffi
    from ampligraph_amd.compat import ComplEx, TransE, evaluate_performance
    from ampligraph_amd.latent_features import loss_functions, optimizers

    m = ComplEx(k=10, eta=3, batches_count=7, optimizer="momentum", optimizer_params={"lr": 0.05},
                initializer="uniform", initializer_params={"low": -0.1, "high": 0.1})
    o = m._get_optimizer()
    assert (o.name, o.keras_name, o.momentum, o.learning_rate) == ("momentum", "sgd", 0.9, 0.05)
    ini = m._get_initializer()
    x = ini((50, 4), np.random.default_rng(0))
    assert x.shape == (50, 4) and -0.1 <= x.min() and x.max() <= 0.1
    assert TransE(initializer="xavier", initializer_params={"uniform": True})._get_initializer() == "glorot_uniform"
    assert TransE()._get_initializer() == "glorot_normal"
    const = TransE(initializer="constant", initializer_params={"entity": np.ones((3, 2)), "relation": np.zeros((1, 2))})._get_initializer()
    assert np.array_equal(const[0]((3, 2), None), np.ones((3, 2), np.float32))
    assert m.get_hyperparameter_dict()["batches_count"] == 7 and not m.is_fit()
    with pytest.raises(AssertionError):
        evaluate_performance(np.zeros((1, 3)), m, corrupt_side="x")
    if not torch.cuda.is_available():
        from ampligraph_amd.session import Session

        with pytest.raises(_ffi.AmdKgeError):
            Session("ComplEx", 8, 10, 2, 3, loss_functions.get("nll"), optimizers.get("adam"))


def test_regulariser_forms_the_reference_accepts():
    """regularizers.get mirrors what the reference hands to tf.keras.regularizers.get (regularizers.py:59-73,
    EmbeddingLookupLayer.py:131-155): LP / l3 with hyper-parameters, Keras' names l1, l2, l1_l2 and the L1L2 config dict; the
    penalty of a table is the sum of at most two LP terms."""
    import numpy as np

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, regularizers

    x = np.array([[1.0, -2.0], [0.5, 0.0]])
    assert regularizers.get(None) is None
    assert regularizers.get("LP").terms == [(2, 1e-5)] and regularizers.get("l3", {"lambda": 0.1}).terms == [(3, 0.1)]
    assert regularizers.get("l1").terms == [(1, 0.01)] and regularizers.get("L2").terms == [(2, 0.01)]
    r = regularizers.get("l1_l2")
    assert r.terms == [(1, 0.01), (2, 0.01)] and abs(r(x) - (0.01 * 3.5 + 0.01 * 5.25)) < 1e-12
    r = regularizers.get({"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.5}})
    assert r.terms == [(2, 0.5)]
    assert regularizers.get({"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.0}}) is None
    with pytest.raises(ValueError):
        regularizers.get("nonsense")
    m = ScoringBasedEmbeddingModel(eta=1, k=4, scoring_type="TransE")
    m.compile(optimizer="adam", loss="nll", entity_relation_regularizer=[regularizers.get("LP", {"p": 3}), None])   # one-sided pair
    assert m._regularizers[0].p == 3 and m._regularizers[1] is None
    with pytest.raises(AssertionError):   # EmbeddingLookupLayer.py:147-150
        m.compile(optimizer="adam", loss="nll", entity_relation_regularizer=["l1", "l2", "l1"])
    from ampligraph_amd.engine import reg_fields

    assert reg_fields(None, 2) == (2, 0.0, 2, 0.0) and reg_fields(0.5, 3) == (3, 0.5, 3, 0.0)
    assert reg_fields(regularizers.get("l1_l2"), 2) == (1, 0.01, 2, 0.01)


def test_session_group_argument_validation_without_gpu():
    """Error paths of the group layer that return before touching a device; the RCCL error class exists."""
    import ctypes

    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    h = ctypes.c_void_p()
    assert lib.amdkge_session_group_create(None, None, 2, ctypes.byref(h)) == -1
    cfg = _ffi.SessionConfig()
    assert lib.amdkge_session_group_create(ctypes.byref(cfg), None, 0, ctypes.byref(h)) == -1
    assert lib.amdkge_session_group_create(ctypes.byref(cfg), None, 17, ctypes.byref(h)) == -1
    assert lib.amdkge_session_group_size(None) == 0
    assert lib.amdkge_session_group_train_step(None, None, 1, None, None) == -1
    # ABI 5: row-sharded evaluation and the column-sharded group
    assert lib.amdkge_session_group_rank(None, None, 1, None, None, None, None, None, 0, 0, 0, None) == -1
    assert lib.amdkge_session_group_create_cols(None, None, 2, 0, ctypes.byref(h)) == -1
    cfg.model.scoring_type, cfg.model.k, cfg.model.n_ents, cfg.model.n_rels = 2, 10, 100, 4
    assert lib.amdkge_session_group_create_cols(ctypes.byref(cfg), None, 4, 0, ctypes.byref(h)) == -1      # k not a multiple of the replicas
    assert b"multiple" in lib.amdkge_last_error()
    cfg.model.k, cfg.model.k_full = 8, 16
    assert lib.amdkge_session_group_create_cols(ctypes.byref(cfg), None, 4, 0, ctypes.byref(h)) == -1      # the config describes the WHOLE model
    cfg.model.k_full = 0
    assert lib.amdkge_session_group_create_cols(ctypes.byref(cfg), None, 4, 1 << 10, ctypes.byref(h)) == -1   # unknown flag
    m = _ffi.Model()
    m.scoring_type, m.k, m.n_ents, m.n_rels, m.k_full = 2, 8, 100, 4, 4
    assert lib.amdkge_cols_partial_scores(ctypes.byref(m), None, None, None, 1, 5, 0, 100, 0, 0, 0, 1, None, None, None) == -1   # k_full < k
    m.k_full = 16
    assert lib.amdkge_cols_partial_scores(ctypes.byref(m), None, None, None, 0, 5, 0, 100, 0, 0, 0, 0, None, None, None) == 0    # an empty batch is a no-op
    assert lib.amdkge_cols_partial_scores(ctypes.byref(m), None, None, None, 1, 5, 0, 100, 0, 0, 0, 1, None, None, None) == -1   # NULL pointers
    # a slice holds up to 256 stored units per half: DistMult's 400-unit rows (the C3 width as a slice of an 800-unit model) are refused
    # before any launch -- host buffers stand in for device memory, no checked path reads them
    m.scoring_type, m.k, m.k_pad, m.k_full, m.n_ents = 1, 400, 400, 800, 5_500_858
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.amdkge_cols_partial_scores(ctypes.byref(m), p, p, p, 1, 5, 0, 100, 0, 0, 0, 1, None, p, None) == -5
    assert b"256 units per half" in lib.amdkge_last_error()
    assert _ffi.ERCCL == -3   # the header's value: tests/test_abi_host.py
