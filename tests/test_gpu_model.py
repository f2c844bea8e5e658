"""End-to-end parity of the drop-in surface (ScoringBasedEmbeddingModel.fit/predict/evaluate) on the GPU
against the oracle replaying the same schedule: same id map, same initial tables, same batches
(sequential slices), same Philox negatives, dense Keras-legacy optimizer."""
import os

import numpy as np
import pytest

from margins import frac_outside, rel_gap, within
from oracle import kge_oracle as O

pytestmark = pytest.mark.gpu


def toy_graph(seed=0, n=700, N=60, R=4):
    rng = np.random.default_rng(seed)
    ents = np.array([f"e{i}" for i in range(N)])
    rels = np.array([f"r{i}" for i in range(R)])
    X = np.stack([ents[rng.integers(0, N, n)], rels[rng.integers(0, R, n)], ents[rng.integers(0, N, n)]], 1)
    return X


def oracle_replay(model, X, k, eta, loss, opt, lr, batch_size, epochs, seed, reg=None, loss_params=None):
    from ampligraph_amd.latent_features.initializers import initialise

    ents, rels = O.first_seen_index(X)
    Xi = O.to_indexes(X, ents, rels)
    N, R = len(ents), len(rels)
    K = O.internal_k(model, k)
    rng = np.random.Generator(np.random.PCG64(seed))
    st = O.TrainState(initialise("glorot_uniform", (N, K), rng), initialise("glorot_uniform", (R, K), rng), opt, lr)
    steps = (len(Xi) + batch_size - 1) // batch_size
    hist = []
    for ep in range(epochs):
        tot = 0.0
        for s in range(steps):
            xb = Xi[s * batch_size:(s + 1) * batch_size]
            tot += float(O.train_step(st, model, xb, eta, loss, seed, ep * steps + s, loss_params=loss_params,
                                      max_rel_size=R, reg=reg))
        hist.append(tot / steps)
    return st, Xi, hist


@pytest.mark.parametrize("model,loss,opt", [("ComplEx", "self_adversarial", "adam"), ("TransE", "pairwise", "sgd"),
                                            ("DistMult", "multiclass_nll", "adagrad"), ("RotatE", "nll", "adam"),
                                            ("HolE", "absolute_margin", "adam"), ("DistMult", "nll", "rmsprop"),
                                            ("ComplEx", "self_adversarial", "adamax"), ("TransE", "pairwise", "adadelta")])
def test_fit_matches_oracle(gpu_lib, model, loss, opt):
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = toy_graph()
    k, eta, bs, epochs, lr = 8, 3, 256, 3, 1e-2
    m = ScoringBasedEmbeddingModel(eta=eta, k=k, scoring_type=model, seed=3)
    from ampligraph_amd.latent_features import optimizers
    m.compile(optimizer=optimizers.get(opt, {"learning_rate": lr}), loss=loss)
    h = m.fit(X, batch_size=bs, epochs=epochs, verbose=False)
    st, Xi, hist = oracle_replay(model, X, k, eta, loss, opt, lr, bs, epochs, seed=3)
    assert np.allclose(h.history["loss"], hist, rtol=2e-4), (h.history["loss"], hist)
    ent = m.get_embeddings(np.array([f"e{i}" for i in range(60)]))
    ref = st.ent[[O.first_seen_index(X)[0][f"e{i}"] for i in range(60)]]
    close = np.abs(ent - ref) <= 1e-4 + 1e-3 * np.abs(ref)
    assert close.mean() > 0.995, close.mean()   # Adam's m/(sqrt(v)+eps) amplifies fp32 noise where g ~ 0
    # predict on the trained tables
    e_all, r_all = m._engine.get_tables()
    sc = m.predict(X[:100])
    s, p, o = O.lookup(e_all, r_all, Xi[:100])
    ref_sc = O.compute_scores(model, s, p, o, max_rel_size=r_all.shape[0])
    assert np.allclose(sc, ref_sc, rtol=1e-5, atol=1e-5 * np.abs(ref_sc).max())


def test_fit_with_lp_regularizer(gpu_lib):
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = toy_graph(1)
    m = ScoringBasedEmbeddingModel(eta=2, k=6, scoring_type="ComplEx", seed=0)
    m.compile(optimizer="adam", loss="multiclass_nll", entity_relation_regularizer="LP",)
    # default LP: p=2, lambda=1e-5 (regularizers.py:35); use a visible lambda through the object form
    from ampligraph_amd.latent_features import regularizers
    m.compile(optimizer="adam", loss="multiclass_nll",
              entity_relation_regularizer=regularizers.get("LP", {"p": 3, "lambda": 1e-2}))
    h = m.fit(X, batch_size=200, epochs=2, verbose=False)
    st, Xi, hist = oracle_replay("ComplEx", X, 6, 2, "multiclass_nll", "adam", 1e-3, 200, 2, 0,
                                 reg={"p": 3, "lam_e": 1e-2, "lam_r": 1e-2})
    assert np.allclose(h.history["loss"], hist, rtol=2e-4)


@pytest.mark.parametrize("model,path", [("ComplEx", "tiled"), ("TransE", "atomic"), ("RotatE", "tiled"), ("DistMult", "lazy")])
@pytest.mark.parametrize("form", ["mixed_p", "entity_only", "relation_only", "l1_l2", "l1_l2_config_and_l3"])
def test_fit_regulariser_forms_of_the_reference(gpu_lib, model, path, form):
    """a17: the reference hands `entity_relation_regularizer` to tf.keras.regularizers.get per table
    (EmbeddingLookupLayer.py:131-155): an [entity, relation] pair of INDEPENDENT regularisers -- different p, either one None --
    and Keras' own names ('l1_l2' = l1 sum|x| + l2 sum x^2).  Loss histories against the oracle with the same per-table terms,
    on the owner-computes pair (fused relation sweep for ComplEx, separate one for RotatE), the atomic path + dense sweep
    (TransE k < 128) and the touched-rows mode."""
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers, regularizers

    LP = lambda p, lam: regularizers.get("LP", {"p": p, "lambda": lam})   # noqa: E731
    pair, terms = {
        "mixed_p": ([LP(3, 2e-2), LP(2, 5e-3)], ([(3, 2e-2)], [(2, 5e-3)])),
        "entity_only": ([LP(2, 1e-2), None], ([(2, 1e-2)], [])),
        "relation_only": ([None, LP(1, 1e-3)], ([], [(1, 1e-3)])),
        "l1_l2": ("l1_l2", ([(1, 0.01), (2, 0.01)], [(1, 0.01), (2, 0.01)])),
        "l1_l2_config_and_l3": ([{"class_name": "L1L2", "config": {"l1": 2e-3, "l2": 3e-2}}, regularizers.get("l3", {"lambda": 1e-2})],
                                ([(1, 2e-3), (2, 3e-2)], [(3, 1e-2)])),
    }[form]
    X = toy_graph(4)
    k, eta, bs, epochs, lr = 8, 3, 256, 3, 1e-2
    m = ScoringBasedEmbeddingModel(eta=eta, k=k, scoring_type=model, seed=2)
    kw = {"optimizer_mode": "lazy"} if path == "lazy" else {}
    m.compile(optimizer=optimizers.get("adam", {"learning_rate": lr}), loss="nll", entity_relation_regularizer=pair, **kw)
    h = m.fit(X, batch_size=bs, epochs=epochs, verbose=False)
    assert m._loop.use_tiled == (path != "atomic")
    reg = {"terms_e": terms[0], "terms_r": terms[1]}
    if path == "lazy":
        st, Xi, hist = lazy_replay(model, X, k, eta, "nll", "adam", lr, bs, epochs, 2, reg)
    else:
        st, Xi, hist = oracle_replay(model, X, k, eta, "nll", "adam", lr, bs, epochs, seed=2, reg=reg)
    assert np.allclose(h.history["loss"], hist, rtol=2e-4), (h.history["loss"], hist)
    ent, rel = m._engine.get_tables()
    for got, ref in ((ent, st.ent), (rel, st.rel)):
        close = np.abs(got - ref) <= 1e-4 + 1e-3 * np.abs(ref)
        assert close.mean() > 0.99, close.mean()


def lazy_replay(model, X, k, eta, loss, opt, lr, batch_size, epochs, seed, reg):
    from ampligraph_amd.latent_features.initializers import initialise

    ents, rels = O.first_seen_index(X)
    Xi = O.to_indexes(X, ents, rels)
    N, R, K = len(ents), len(rels), O.internal_k(model, k)
    rng = np.random.Generator(np.random.PCG64(seed))
    st = O.TrainState(initialise("glorot_uniform", (N, K), rng), initialise("glorot_uniform", (R, K), rng), opt, lr)
    steps = -(-len(Xi) // batch_size)
    hist = []
    for ep in range(epochs):
        tot = 0.0
        for s_ in range(steps):
            tot += float(O.train_step(st, model, Xi[s_ * batch_size:(s_ + 1) * batch_size], eta, loss, seed, ep * steps + s_,
                                      max_rel_size=R, reg=reg, lazy=True))
        hist.append(tot / steps)
    return st, Xi, hist


@pytest.mark.parametrize("model", ["ComplEx", "TransE", "RotatE"])
def test_evaluate_matches_oracle(gpu_lib, model):
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = toy_graph(2, n=900)
    train, test = X[:800], X[800:]
    m = ScoringBasedEmbeddingModel(eta=3, k=8, scoring_type=model, seed=1)
    m.compile(optimizer="adam", loss="nll")
    m.fit(train, batch_size=300, epochs=2, verbose=False)
    ents, rels = O.first_seen_index(train)
    ti = O.to_indexes(test, ents, rels)
    tri = O.to_indexes(train, ents, rels)
    ent, rel = m._engine.get_tables()
    R = rel.shape[0]
    cases = [
        dict(use_filter=False, corrupt_side="s,o", strat="worst", fl=None, sub=None),
        dict(use_filter=True, corrupt_side="s,o", strat="worst", fl=[ti], sub=None),
        dict(use_filter={"train": train, "test": test}, corrupt_side="s,o", strat="middle", fl=[tri, ti], sub=None),
        dict(use_filter={"train": train, "test": test}, corrupt_side="s", strat="best", fl=[tri, ti], sub=None),
        dict(use_filter={"train": train, "test": test}, corrupt_side="o", strat="worst", fl=[tri, ti], sub=None),
        dict(use_filter={"train": train, "test": test}, corrupt_side="s+o", strat="worst", fl=[tri, ti], sub=None),
        dict(use_filter={"train": train}, corrupt_side="s,o", strat="worst", fl=[tri], sub=[f"e{i}" for i in range(0, 60, 3)]),
    ]
    for c in cases:
        got = m.evaluate(test, use_filter=c["use_filter"], corrupt_side=c["corrupt_side"],
                         ranking_strategy=c["strat"], entities_subset=c["sub"], verbose=False)
        fs = fo = None
        if c["fl"] is not None:
            fs, fo = O.filter_sets(ti, c["fl"])
        sub_idx = None
        if c["sub"] is not None:
            sub_idx = [ents[e] for e in c["sub"] if e in ents]
        ref = O.evaluate_ranks(model, ent, rel, ti, fs if "s" in c["corrupt_side"] else None,
                               fo if "o" in c["corrupt_side"] else None, c["corrupt_side"], c["strat"],
                               entities_subset=sub_idx, max_rel_size=R)
        assert got.shape == ref.shape and got.dtype == np.int32
        # fragile-aware comparison (fp32 order noise at the 1e-3 truncation boundary)
        E = ent if sub_idx is None else ent[np.asarray(sub_idx)]
        frag = sum(O.fragile_rank_mask(model, ent, rel, ti, sd, max_rel_size=R, ent_matrix=E)
                   for sd in ("s", "o") if sd in c["corrupt_side"])
        diff = np.abs(got.astype(np.int64) - ref).sum(1)
        assert (diff <= 2 * frag).all(), (model, c["corrupt_side"], c["strat"], diff.max())
        assert (diff > 0).mean() < 0.05


def test_api_errors_and_dropped_rows(gpu_lib):
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = toy_graph(3, n=300)
    m = ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type="DistMult")
    with pytest.raises(RuntimeError):
        m.fit(X, epochs=1)                      # compile first (:713)
    m.compile(optimizer="adam", loss="pairwise")
    with pytest.raises(AssertionError):
        m.predict(X[:3])                        # not fitted
    m.fit(X, batch_size=100, epochs=1, verbose=False)
    with pytest.raises(AssertionError):
        m.evaluate(X[:5], corrupt_side="x")     # :1605-1610
    with pytest.raises(AssertionError):
        m.evaluate(X[:5], ranking_strategy="median")
    bad = np.array([["e0", "r0", "nope"], X[0], ["e1", "zz", "e2"]])
    assert m.predict(bad).shape == (1,)         # unknown keys silently dropped (data_indexer.py:526-542)
    assert m.evaluate(bad, verbose=False).shape == (1, 2)
    assert m.get_count("e") == len(set(X[:, 0]) | set(X[:, 2])) and m.get_count("r") == len(set(X[:, 1]))
    with pytest.raises(ValueError):
        m.get_count("x")
    assert m.get_embeddings(["e0", "e1"]).shape == (2, 4)
    assert m.get_embeddings(["r0"], "r").shape == (1, 4)
    assert m.is_fit()


def test_save_load_weights_roundtrip(gpu_lib, tmp_path):
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = toy_graph(4, n=300)
    m = ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type="ComplEx", seed=2)
    m.compile(optimizer="adam", loss="nll")
    m.fit(X, batch_size=100, epochs=2, verbose=False)
    p = str(tmp_path / "w")
    m.save_weights(p)
    m2 = ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type="ComplEx", seed=2)
    m2.compile(optimizer="adam", loss="nll")
    m2.load_weights(p)
    assert np.array_equal(m.predict(X[:50]), m2.predict(X[:50]))
    assert np.array_equal(m.evaluate(X[:20], use_filter=True, verbose=False), m2.evaluate(X[:20], use_filter=True, verbose=False))
    # resumed training continues identically (tables + Adam slots + iteration counter restored)
    h1 = m.fit(X, batch_size=100, epochs=3, initial_epoch=2, verbose=False)
    h2 = m2.fit(X, batch_size=100, epochs=3, initial_epoch=2, verbose=False)
    # (same code from bit-equal state, but k = 4 takes the atomic path: fp32 arrival order -- see tests/margins.py)
    assert within("model/resume_same_state/loss", rel_gap(h1.history["loss"], h2.history["loss"]), 2e-5)


# ------------------------------------------------------------------------------------ row-sharded mode
@pytest.mark.parametrize("model,k,negatives", [("ComplEx", 8, "global"), ("TransE", 12, "global"), ("DistMult", 7, "global"),
                                               ("ComplEx", 8, "local")])
def test_row_sharded_engines_on_one_gpu(gpu_lib, model, k, negatives):
    """ampligraph_amd/sharded.py driving TWO real KgeEngines (half the entity table each, scratch rows behind the
    shard) through an in-process rendezvous (tests/threaded_dist.py).  negatives="global": == one engine with the
    whole table (same Philox corruptions).  negatives="local": == the oracle restatement of shard-local sampling.
    Also the sharded evaluation: partial counts summed over shards == whole-table ranks."""
    import torch
    from threaded_dist import ThreadedWorld

    from ampligraph_amd import _ffi
    from ampligraph_amd.engine import KgeEngine
    from ampligraph_amd.latent_features import loss_functions, optimizers, regularizers
    from ampligraph_amd.sharded import ShardedStepLoop, ShardSpec, sharded_rank_counts
    from ampligraph_amd.trainer import StepLoop, shard_bounds

    rng = np.random.default_rng(2)
    N, R, eta, bs, seed, W = 83, 4, 3, 64, 11, 2
    K = O.internal_k(model, k)
    ent = (rng.normal(size=(N, K)) * 0.4).astype(np.float32)
    rel = (rng.normal(size=(R, K)) * 0.4).astype(np.float32)
    X = np.stack([rng.integers(0, N, 200), rng.integers(0, R, 200), rng.integers(0, N, 200)], 1).astype(np.int32)
    mk = lambda: (loss_functions.get("self_adversarial"), optimizers.get("adam", {"learning_rate": 1e-2}),
                  regularizers.get("LP", {"p": 2, "lambda": 1e-3}))
    T = X[:40]

    def body(dist):
        sp = ShardSpec(N, W, dist.get_rank())
        cap = ShardedStepLoop.rows_needed(bs, eta, negatives) + 2 * len(T)
        eng = KgeEngine(model, k, sp.n_local + cap, R, max_rel_size=R)
        shard = np.zeros((sp.n_local + cap, K), dtype=np.float32)
        shard[:sp.n_local] = ent[sp.lo:sp.hi]
        eng.set_tables(shard, rel)
        loss, opt, reg = mk()
        loop = ShardedStepLoop(eng, sp, eta, loss, opt, reg, seed, dist, negatives=negatives)
        Xt = torch.as_tensor(X).cuda()
        loop.reset_loss()
        step = 0
        for ep in range(2):
            for b0 in range(0, len(X), bs):
                loop.step(Xt[b0:b0 + bs], step)
                step += 1
        lossv = loop.mean_batch_loss()
        full = eng.unpack(loop.gather_entity_table()).cpu().numpy()
        cs, _ = sharded_rank_counts(eng, sp, dist, torch.as_tensor(T).cuda(), _ffi.SIDE_S)
        co, _ = sharded_rank_counts(eng, sp, dist, torch.as_tensor(T).cuda(), _ffi.SIDE_O)
        return full, eng.unpack(eng.rel).cpu().numpy(), lossv, cs.cpu().numpy(), co.cpu().numpy()

    res = ThreadedWorld(W).run(body)
    full, relg, lossv, cs, co = res[0]
    assert np.array_equal(full, res[1][0]) and np.array_equal(relg, res[1][1])   # replicas agree

    if negatives == "global":   # one engine, whole table, same schedule
        eng1 = KgeEngine(model, k, N, R, max_rel_size=R)
        eng1.set_tables(ent, rel)
        loss, opt, reg = mk()
        loop1 = StepLoop(eng1, eta, loss, opt, reg, seed, None)
        Xt = torch.as_tensor(X).cuda()
        loop1.reset_loss()
        step = 0
        for ep in range(2):
            for b0 in range(0, len(X), bs):
                loop1.step(Xt[b0:b0 + bs], step)
                step += 1
        e1, r1 = eng1.get_tables()
        ref_loss = loop1.mean_batch_loss()
    else:
        st = O.TrainState(ent, rel, "adam", 1e-2)
        specs = [ShardSpec(N, W, r) for r in range(W)]
        step, tot, ns = 0, 0.0, 0
        for ep in range(2):
            for b0 in range(0, len(X), bs):
                xb = X[b0:b0 + bs]
                Ge, Gr = np.zeros(ent.shape), np.zeros(rel.shape)
                for r in range(W):
                    lo, hi = shard_bounds(len(xb), W, r)
                    xr, sp = xb[lo:hi], specs[r]
                    B = len(xr)
                    j = np.repeat(np.arange(eta, dtype=np.uint64), B)
                    i = np.tile(np.arange(B, dtype=np.uint64), eta)
                    keep, repl = O.sample_corruption_draws(j * np.uint64(len(xb)) + np.uint64(lo) + i, step, seed, sp.n_local)
                    data = np.tile(xr, (eta, 1))
                    repl = repl.astype(np.int64) + sp.lo
                    ng = np.stack([np.where(keep == 1, data[:, 0], repl), data[:, 1], np.where(keep == 1, repl, data[:, 2])], 1)
                    l, ge, gr, _ = O.dense_gradients(model, st.ent, st.rel, xr, ng, eta, "self_adversarial", None, "sum", R)
                    Ge += ge; Gr += gr; tot += float(l)
                for x, G in ((st.ent, Ge), (st.rel, Gr)):
                    xx = x.astype(np.float64)
                    tot += 1e-3 * float((xx ** 2).sum())
                    G += 2e-3 * xx
                O.apply_optimizer(st, Ge, Gr)
                step += 1
                ns += 1
        e1, r1, ref_loss = st.ent, st.rel, tot / ns
    close = np.abs(full - e1) <= 1e-5 + 1e-3 * np.abs(e1)
    assert close.mean() > 0.995, close.mean()
    assert np.abs(full - e1).max() < 2.5e-2 and np.abs(relg - r1).max() < 2.5e-2
    assert abs(lossv - ref_loss) <= 2e-4 * abs(ref_loss), (lossv, ref_loss)
    # sharded evaluation == one engine holding the gathered table
    engf = KgeEngine(model, k, N, R, max_rel_size=R)
    engf.set_tables(full, relg)
    Td = torch.as_tensor(T).cuda()
    for side, got in ((_ffi.SIDE_S, cs), (_ffi.SIDE_O, co)):
        ref = engf.rank_side(Td, side, "worst")[1].cpu().numpy()
        assert np.array_equal(got, ref), side


def test_model_row_sharded_matches_single_gpu(gpu_lib):
    """Drop-in surface in row-sharded mode (compile(entity_sharding="rows")): two model replicas (threads, in-process
    rendezvous) holding half the entity table each == one model on one GPU: loss history, embeddings, predict,
    filtered evaluate.  sharded_negatives="global" draws the single-GPU corruptions, so the runs are comparable."""
    from threaded_dist import ThreadedWorld

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers
    from ampligraph_amd.placement import Rows

    X = toy_graph(n=600, N=50, R=3)
    Xtest = X[:60]
    k, eta, bs, epochs = 8, 3, 128, 3

    def make():
        m = ScoringBasedEmbeddingModel(eta=eta, k=k, scoring_type="ComplEx", seed=4)
        return m

    def body(dist):
        m = make()
        m._dist_override = dist
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="self_adversarial",
                  entity_relation_regularizer="l2", entity_sharding="rows", sharded_negatives="global")
        h = m.fit(X, batch_size=bs, epochs=epochs, verbose=False)
        assert isinstance(m._placement, Rows) and m._engine.ent.shape[0] < 50 + 2 * m.EVAL_CHUNK_SHARDED + 1000
        ents = np.array([f"e{i}" for i in range(50)])
        return (h.history["loss"], m.get_embeddings(ents), m.predict(Xtest),
                m.evaluate(Xtest, use_filter={"train": X}, corrupt_side="s,o", verbose=False),
                m.evaluate(Xtest, corrupt_side="s+o", ranking_strategy="middle", verbose=False))

    res = ThreadedWorld(2).run(body)
    m1 = make()
    m1.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="self_adversarial",
               entity_relation_regularizer="l2")
    h1 = m1.fit(X, batch_size=bs, epochs=epochs, verbose=False)
    ents = np.array([f"e{i}" for i in range(50)])
    e1, p1 = m1.get_embeddings(ents), m1.predict(Xtest)
    for hist, emb, pred, rf, rm in res:
        assert np.allclose(hist, h1.history["loss"], rtol=2e-4)
        close = np.abs(emb - e1) <= 1e-5 + 1e-3 * np.abs(e1)
        assert close.mean() > 0.995
        assert np.allclose(pred, p1, rtol=1e-3, atol=1e-4)
    # the two replicas agree exactly with each other; ranks are compared on THEIR (gathered) tables
    assert np.array_equal(res[0][3], res[1][3]) and np.array_equal(res[0][4], res[1][4])
    m1._engine.set_tables(_reorder(res[0][1], m1, ents), m1._engine.get_tables()[1])
    # relation tables differ by fp32 summation order only; compare ranks up to that noise
    rf1 = m1.evaluate(Xtest, use_filter={"train": X}, corrupt_side="s,o", verbose=False)
    assert (np.abs(rf1 - res[0][3]) <= 1).mean() > 0.97


def _reorder(emb_by_name, model, ents):
    """embeddings listed by entity name -> table order of `model`'s indexer"""
    idx = model.data_indexer.get_indexes(ents, "e")
    tab = np.zeros_like(emb_by_name)
    tab[idx] = emb_by_name
    return tab


# ------------------------------------------------------------------------------------ calibration (8f.3)
def test_platt_kernel_parity(gpu_lib):
    import torch

    from ampligraph_amd.engine import KgeEngine

    eng = KgeEngine("DistMult", 4, 5, 2)
    rng = np.random.default_rng(3)
    for npos, nneg in ((3, 3), (1000, 257), (5, 4000)):
        sp = rng.normal(size=npos).astype(np.float32) * 3
        sn = rng.normal(size=nneg).astype(np.float32) * 3 - 1
        _, _, labels, neg_size, rate = O.platt_init(npos, nneg)
        for w, b in ((0.0, 0.3), (-1.5, 0.2), (10.0, 10.0)):
            got = eng.platt_step(torch.as_tensor(sp).cuda(), torch.as_tensor(sn).cuda(), w, b, labels[0], labels[1],
                                 nneg / npos, (1 - rate) / rate)
            ref = O.platt_loss_and_grads(sp, sn, w, b, labels, rate)
            assert np.allclose(got, ref, rtol=2e-5, atol=1e-6), (npos, nneg, w, b, got, ref)
    # the reference's own KAT through the kernel (test_calibrate.py:39-51)
    got = eng.platt_step(torch.tensor([-2., 1., -1.]).cuda(), torch.tensor([10., 11., 12.]).cuda(), 10, 10, 6 / 7, 1 / 7, 1.0, 1.0)
    assert np.around(np.float32(got[0]), 2) == np.float32(11.78)


@pytest.mark.parametrize("with_negatives", [True, False])
def test_calibrate_matches_oracle(gpu_lib, with_negatives):
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = toy_graph(n=500, N=40, R=3)
    m = ScoringBasedEmbeddingModel(eta=2, k=8, scoring_type="ComplEx", seed=1)
    m.compile(optimizer="adam", loss="nll")
    with pytest.raises(RuntimeError):
        m.is_fitted = True
        m.data_indexer = None
        m.predict_proba(X[:3])
    m.is_fitted = False
    m.fit(X, batch_size=100, epochs=2, verbose=False)
    Xp = X[:90]
    rng = np.random.default_rng(5)
    Xn = X[rng.permutation(len(X))[:140]].copy()
    Xn[:, 2] = X[rng.integers(0, len(X), 140), 2]
    bs, epochs = 32, 3
    if with_negatives:
        m.calibrate(Xp, Xn, batch_size=bs, epochs=epochs)
    else:
        with pytest.raises(AssertionError):
            m.calibrate(Xp, batch_size=bs, epochs=epochs)
        with pytest.raises(ValueError):
            m.calibrate(Xp, positive_base_rate=1.5)
        m.calibrate(Xp, positive_base_rate=0.3, batch_size=bs, epochs=epochs)
    # oracle replay on the same scores
    sp_all = m.predict(Xp)
    npos = len(Xp)
    if with_negatives:
        sn_all, nneg = m.predict(Xn), len(Xn)
        w, b, labels, _, rate = O.platt_init(npos, nneg)
    else:
        w, b, labels, _, rate = O.platt_init(npos, positive_base_rate=0.3)
    nb = -(-npos // bs)
    bsn = bs if not with_negatives or -(-len(Xn) // bs) == nb else -(-len(Xn) // nb)
    e_all, r_all = m._engine.get_tables()
    Xpi = m.data_indexer.get_indexes(Xp)
    slots, t = [(0.0, 0.0), (0.0, 0.0)], 0
    for ep in range(epochs):
        for bi in range(nb):
            sp = sp_all[bi * bs:(bi + 1) * bs]
            if with_negatives:
                sn = sn_all[bi * bsn:(bi + 1) * bsn]
            else:
                neg = O.generate_corruptions(Xpi[bi * bs:(bi + 1) * bs], e_all.shape[0], 1, 1, t)
                sn = O.compute_scores("ComplEx", *O.lookup(e_all, r_all, neg), max_rel_size=r_all.shape[0])
            t += 1
            _, gw, gb = O.platt_loss_and_grads(sp, sn, w, b, labels, rate)
            w, b = O.adam_scalar_step([w, b], [gw, gb], slots, t)
    cp = m.calibration_parameters
    assert abs(cp["calib_w"] - w) < 2e-5 and abs(cp["calib_b"] - b) < 2e-5, (cp, w, b)
    pr = m.predict_proba(Xp)
    assert np.allclose(pr, O.platt_proba(sp_all, cp["calib_w"], cp["calib_b"]), atol=1e-6)
    assert pr.min() > 0 and pr.max() < 1


# ------------------------------------------------------------------------------------ FocusE through fit()
@pytest.mark.parametrize("model,nl,stop", [("ComplEx", "sigmoid", 4), ("TransE", "linear", 0), ("DistMult", "softplus", 251)])
def test_fit_focuse_matches_oracle(gpu_lib, model, nl, stop):
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers

    X = toy_graph(n=400, N=40, R=3)
    rng = np.random.default_rng(8)
    W = rng.random((len(X), 2)).astype(np.float32)
    X4 = np.concatenate([X, W.astype(str)], 1)
    k, eta, bs, epochs, lr = 8, 3, 128, 3, 1e-2
    m = ScoringBasedEmbeddingModel(eta=eta, k=k, scoring_type=model, seed=6)
    m.compile(optimizer=optimizers.get("adam", {"learning_rate": lr}), loss="nll")
    fp = {"non_linearity": nl, "stop_epoch": stop, "structural_wt": 0.3}
    h = m.fit(X4, batch_size=bs, epochs=epochs, verbose=False, focusE=True, focusE_params=fp)
    with pytest.raises(ValueError):
        m.fit(X4, batch_size=bs, epochs=1, verbose=False, focusE=True, focusE_params={"non_linearity": "relu"})
    # oracle replay with the same schedule
    from ampligraph_amd.latent_features.initializers import initialise

    ents, rels = O.first_seen_index(X)
    Xi = O.to_indexes(X, ents, rels)
    N, R, K = len(ents), len(rels), O.internal_k(model, k)
    rg = np.random.Generator(np.random.PCG64(6))
    st = O.TrainState(initialise("glorot_uniform", (N, K), rg), initialise("glorot_uniform", (R, K), rg), "adam", lr)
    wmean = W.astype(np.float32).mean(axis=1)
    steps = -(-len(Xi) // bs)
    hist = []
    for ep in range(epochs):
        beta = max(1.0 - ep / stop, 0.001) if stop > 0 else 0.3
        tot = 0.0
        for s_ in range(steps):
            sl = slice(s_ * bs, (s_ + 1) * bs)
            tot += float(O.train_step(st, model, Xi[sl], eta, "nll", 6, ep * steps + s_, max_rel_size=R,
                                      focus=(wmean[sl], beta, nl)))
        hist.append(tot / steps)
    assert np.allclose(h.history["loss"], hist, rtol=3e-4), (h.history["loss"], hist)
    e_all, _ = m._engine.get_tables()
    close = np.abs(e_all - st.ent) <= 1e-4 + 1e-3 * np.abs(st.ent)
    assert close.mean() > 0.99, close.mean()
    # 3-column data with focusE=True: silently off, like the reference (:767-768)
    m2 = ScoringBasedEmbeddingModel(eta=eta, k=k, scoring_type=model, seed=6)
    m2.compile(optimizer="adam", loss="nll")
    m2.fit(X, batch_size=bs, epochs=1, verbose=False, focusE=True)
    assert m2.use_focusE is False


# ------------------------------------------------------------------------------------ discovery helpers, callbacks (8f)
def test_query_topn_and_neighbours(gpu_lib):
    """The reference's own test_query_topn (tests/ampligraph/discovery/test_discovery.py:238-313) + parity with predict."""
    from ampligraph_amd.discovery import find_nearest_neighbours, query_topn
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = np.array([['a', 'y', 'b'], ['b', 'y', 'a'], ['a', 'y', 'c'], ['c', 'y', 'a'], ['a', 'y', 'd'], ['c', 'x', 'd'],
                  ['b', 'y', 'c'], ['f', 'y', 'e'], ['a', 'z', 'f'], ['c', 'z', 'f'], ['b', 'z', 'f']])
    model = ScoringBasedEmbeddingModel(eta=5, k=10, scoring_type='ComplEx')
    model.compile(optimizer='adam', loss='multiclass_nll')
    with pytest.raises(ValueError):   # model not fitted
        query_topn(model, top_n=2)
    model.fit(X, batch_size=2, epochs=10, verbose=False)
    bad = [dict(), dict(head='a'), dict(relation='y'), dict(tail='e'), dict(head='a', relation='y', tail='e'),
           dict(head='xx', relation='y'), dict(head='a', relation='yakkety'), dict(head='a', tail='sax'),
           dict(head='a', relation='x', rels_to_consider=['y', 'z']), dict(head='a', tail='f', rels_to_consider=['y', 'z', 'error']),
           dict(head='a', tail='e', rels_to_consider='y'), dict(head='a', relation='x', ents_to_consider=['zz', 'top']),
           dict(head='a', tail='e', ents_to_consider=['a', 'b'])]
    for kw in bad:
        with pytest.raises(ValueError):
            query_topn(model, top_n=2, **kw)
    subj, pred, obj, top_n = 'a', 'x', 'e', 3
    Y, S = query_topn(model, top_n=top_n, head=subj, relation=pred)
    assert len(Y) == len(S) == top_n and np.all(Y[:, 0] == subj) and np.all(Y[:, 1] == pred)
    Y, S = query_topn(model, top_n=top_n, relation=pred, tail=obj)
    assert np.all(Y[:, 1] == pred) and np.all(Y[:, 2] == obj)
    ents_to_con = ['a', 'b', 'c', 'd']
    Y, S = query_topn(model, top_n=top_n, relation=pred, tail=obj, ents_to_consider=ents_to_con)
    assert np.all([x in ents_to_con for x in Y[:, 0]])
    Y, S = query_topn(model, top_n=100, head=subj, tail=obj, rels_to_consider=['y', 'x'])
    assert np.all([x in ['y', 'x'] for x in Y[:, 1]])
    Y, S = query_topn(model, top_n=100, relation=pred, tail=obj)
    assert all(S[i] >= S[i + 1] for i in range(len(S) - 1))
    assert np.allclose(S, model.predict(Y), rtol=1e-5, atol=1e-6)   # same scores as the predict path on the returned triples (fp32 summation order differs)
    nb, dist = find_nearest_neighbours(model, ['b'], n_neighbors=3, entities_subset=['a', 'c', 'd', 'e', 'f'])
    emb = model.get_embeddings(['a', 'c', 'd', 'e', 'f']).astype(np.float64)
    d_ref = np.sort(np.linalg.norm(emb - model.get_embeddings(['b']).astype(np.float64), axis=1))[:3]
    assert nb.shape == (1, 3) and np.allclose(dist[0], d_ref, rtol=1e-5)


def test_early_stopping_callback(gpu_lib):
    from ampligraph_amd.callbacks import EarlyStopping
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = toy_graph(n=400, N=40, R=3)
    m = ScoringBasedEmbeddingModel(eta=2, k=8, scoring_type="DistMult", seed=2)
    m.compile(optimizer="adam", loss="nll")
    es = EarlyStopping(monitor="val_mrr", patience=1, restore_best_weights=True)
    h = m.fit(X[:300], batch_size=100, epochs=50, verbose=False, validation_data=X[300:], validation_freq=2,
              validation_batch_size=100, callbacks=[es])
    assert len(h.history["loss"]) < 50 and m.stop_training and "val_mrr" in h.history
    es2 = EarlyStopping(monitor="loss", patience=3, min_delta=1e9)   # nothing ever improves by 1e9: stops after `patience` epochs
    h2 = m.fit(X[:300], batch_size=100, epochs=50, verbose=False, callbacks=[es2])
    assert len(h2.history["loss"]) <= 5


def test_replicated_evaluate_splits_queries_over_ranks(gpu_lib):
    """Replicated tables, 2 ranks (in-process rendezvous): evaluate() splits the test triples over the ranks and
    gathers; every rank returns exactly the single-GPU ranks (incl. use_filter=True, which must keep filtering with the
    whole evaluated set)."""
    from threaded_dist import ThreadedWorld

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = toy_graph(n=500, N=50, R=3)
    Xt = X[:77]

    def make(dist=None):
        m = ScoringBasedEmbeddingModel(eta=2, k=8, scoring_type="DistMult", seed=3)
        m._dist_override = dist
        m.compile(optimizer="adam", loss="nll")
        m.fit(X, batch_size=128, epochs=2, verbose=False)
        return m

    sums = []
    m1 = make()
    ref = [m1.evaluate(Xt, use_filter=True, corrupt_side="s,o", verbose=False),
           m1.evaluate(Xt, use_filter={"train": X}, corrupt_side="s+o", ranking_strategy="middle", verbose=False),
           m1.evaluate(Xt, corrupt_side="o", verbose=False)]
    e1, r1 = m1._engine.get_tables()

    def body(dist):
        m = make(dist)
        # data-parallel fit of two replicas (sharded merge: all_to_all reduce-scatter, sharded Adam sweep, all_gather of
        # the parameters) == the single-GPU fit up to fp32 summation order, and the replicas hold identical tables
        assert m._loop.merge == "sharded" and m._loop.world == 2
        ed, rd = m._engine.get_tables()
        assert np.allclose(m.history.history["loss"], m1.history.history["loss"], rtol=2e-4)
        assert np.mean(np.abs(ed - e1) <= 1e-5 + 1e-3 * np.abs(e1)) > 0.995 and np.abs(rd - r1).max() < 2.5e-2
        sums.append((float(np.abs(ed).sum()), float(np.abs(rd).sum())))
        # checkpoint from a data-parallel run: the sharded optimizer slots are exchanged first, so every rank writes the
        # same complete Adam state as the single-GPU run holds
        m._loop.sync_optimizer_slots()
        for nme in ("m_e", "v_e", "m_r", "v_r"):
            a_, b_ = m._engine.unpack(m._engine.slots[nme]).cpu().numpy(), m1._engine.unpack(m1._engine.slots[nme]).cpu().numpy()
            assert np.allclose(a_, b_, rtol=2e-3, atol=1e-7), nme
        m._engine.set_tables(e1, r1)   # identical tables: DP training differs only by fp32 summation order
        return [m.evaluate(Xt, use_filter=True, corrupt_side="s,o", verbose=False),
                m.evaluate(Xt, use_filter={"train": X}, corrupt_side="s+o", ranking_strategy="middle", verbose=False),
                m.evaluate(Xt, corrupt_side="o", verbose=False)]

    for got in ThreadedWorld(2).run(body):
        for a, b in zip(got, ref):
            assert a.shape == b.shape and np.array_equal(a, b)
    assert len(sums) == 2 and sums[0] == sums[1]


def test_fit_validation_split_and_separate_lambdas(gpu_lib):
    """validation_split (train_test_split_no_unseen inside fit, :719-728) and an [entity, relation] regulariser pair with
    different lambdas, against the oracle replay on the same split."""
    from ampligraph_amd.evaluation import train_test_split_no_unseen
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers, regularizers

    X = toy_graph(n=500, N=40, R=3)
    k, eta, bs, epochs, lr = 8, 3, 128, 2, 1e-2
    m = ScoringBasedEmbeddingModel(eta=eta, k=k, scoring_type="ComplEx", seed=9)
    regs = [regularizers.get("LP", {"p": 2, "lambda": 1e-3}), regularizers.get("LP", {"p": 2, "lambda": 5e-2})]
    m.compile(optimizer=optimizers.get("adam", {"learning_rate": lr}), loss="nll", entity_relation_regularizer=regs)
    h = m.fit(X, batch_size=bs, epochs=epochs, verbose=False, validation_split=0.1, validation_freq=1, validation_batch_size=64)
    assert "val_mrr" in h.history and len(h.history["val_mrr"]) == epochs
    Xtr, Xva = train_test_split_no_unseen(X, test_size=0.1, seed=9)
    assert m.get_count("e") == len(set(Xtr[:, 0]) | set(Xtr[:, 2]))
    st, Xi, hist = oracle_replay_reg("ComplEx", Xtr, k, eta, "nll", "adam", lr, bs, epochs, 9, dict(p=2, lam_e=1e-3, lam_r=5e-2))
    assert np.allclose(h.history["loss"], hist, rtol=3e-4), (h.history["loss"], hist)


def oracle_replay_reg(model, X, k, eta, loss, opt, lr, batch_size, epochs, seed, reg):
    from ampligraph_amd.latent_features.initializers import initialise

    ents, rels = O.first_seen_index(X)
    Xi = O.to_indexes(X, ents, rels)
    N, R, K = len(ents), len(rels), O.internal_k(model, k)
    rng = np.random.Generator(np.random.PCG64(seed))
    st = O.TrainState(initialise("glorot_uniform", (N, K), rng), initialise("glorot_uniform", (R, K), rng), opt, lr)
    steps = -(-len(Xi) // batch_size)
    hist = []
    for ep in range(epochs):
        tot = 0.0
        for s_ in range(steps):
            tot += float(O.train_step(st, model, Xi[s_ * batch_size:(s_ + 1) * batch_size], eta, loss, seed, ep * steps + s_,
                                      max_rel_size=R, reg=reg))
        hist.append(tot / steps)
    return st, Xi, hist


def test_filter_index_cache(gpu_lib):
    """evaluate() caches the filter index by content: same datasets -> same object and same ranks; changed content or a
    new fit (new id map) -> rebuilt."""
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = toy_graph(n=400, N=40, R=3)
    m = ScoringBasedEmbeddingModel(eta=2, k=8, scoring_type="DistMult", seed=1)
    m.compile(optimizer="adam", loss="nll")
    m.fit(X[:300], batch_size=100, epochs=1, verbose=False)
    flt = {"train": X[:300], "test": X[300:]}
    r1 = m.evaluate(X[300:], use_filter=flt, verbose=False)
    fi1 = m._filter_cache[1]
    r2 = m.evaluate(X[300:], use_filter={"a": X[:300].copy(), "b": X[300:].copy()}, verbose=False)   # equal content, new arrays
    assert m._filter_cache[1] is fi1 and np.array_equal(r1, r2)
    X2 = X.copy()
    X2[0, 2] = X2[1, 2]
    m.evaluate(X[300:], use_filter={"train": X2[:300], "test": X[300:]}, verbose=False)
    assert m._filter_cache[1] is not fi1
    m.fit(X[:300], batch_size=100, epochs=1, verbose=False)   # continue training keeps the id map ...
    m2 = ScoringBasedEmbeddingModel(eta=2, k=8, scoring_type="DistMult", seed=1)
    m2.compile(optimizer="adam", loss="nll")
    m2.fit(X[:200], batch_size=100, epochs=1, verbose=False)
    assert m2._filter_cache == (None, None)                   # ... a new model starts empty


def test_compat_1x_api(gpu_lib):
    """ampligraph_amd.compat (the reference's compat/models.py + compat/evaluate.py surface): argument mapping onto the
    engine -- same result as driving ScoringBasedEmbeddingModel directly with the mapped arguments."""
    from ampligraph_amd.compat import ComplEx, evaluate_performance
    from ampligraph_amd.evaluation import hits_at_n_score, mrr_score
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers, regularizers

    X = toy_graph(n=500, N=40, R=3)
    tr, te = X[:400], X[400:]
    cm = ComplEx(batches_count=4, epochs=3, k=8, eta=3, seed=5, loss="self_adversarial", loss_params={"margin": 2.0, "alpha": 0.3},
                 optimizer="adam", optimizer_params={"lr": 1e-2}, regularizer="LP", regularizer_params={"p": 3, "lambda": 1e-4},
                 initializer="xavier", initializer_params={"uniform": True})
    cm.fit(tr)
    assert cm.is_fit() and cm.get_count("entity") == len(set(tr[:, 0]) | set(tr[:, 2]))
    ranks = evaluate_performance(te, cm, filter_triples=X, corrupt_side="s,o")
    m = ScoringBasedEmbeddingModel(eta=3, k=8, scoring_type="ComplEx", seed=5)
    from ampligraph_amd.latent_features import loss_functions

    m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}),
              loss=loss_functions.get("self_adversarial", {"margin": 2.0, "alpha": 0.3}),
              entity_relation_initializer="glorot_uniform",
              entity_relation_regularizer=regularizers.get("LP", {"p": 3, "lambda": 1e-4}))
    m.fit(tr, batch_size=100, epochs=3, verbose=False)
    ref = m.evaluate(te, use_filter={"valid": X}, corrupt_side="s,o", verbose=False)
    assert np.allclose(cm.predict(te), m.predict(te), rtol=1e-4, atol=1e-6)
    assert (np.abs(ranks - ref) <= 1).mean() > 0.97 and 0 < mrr_score(ranks) <= 1 and 0 <= hits_at_n_score(ranks, 10) <= 1
    assert cm.get_embeddings(["e1", "e2"], "entity").shape == (2, 16)
    assert cm.get_hyperparameter_dict()["batches_count"] == 4
    with pytest.raises(ValueError):
        evaluate_performance(te, cm, filter_triples="nope")


def test_row_sharded_focuse_calibrate_subset_checkpoint(gpu_lib, tmp_path):
    """Row-sharded drop-in class, the rest of the surface: FocusE fit, calibrate/predict_proba, evaluate with
    entities_subset, and the sharded checkpoint (per-rank shard files, no gather): written by 2 ranks, resumed by ONE
    model (re-sliced) and by 2 ranks again -- the continued runs equal the uninterrupted ones."""
    from threaded_dist import ThreadedWorld

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers

    X = toy_graph(n=600, N=50, R=3)
    rng = np.random.default_rng(3)
    Xw = np.concatenate([X, rng.uniform(0, 1, size=(len(X), 1)).astype(str)], 1)
    Xtest = X[:60]
    subset = np.array([f"e{i}" for i in (3, 44, 17, 9, 3, 30, 31, 48)])
    k, eta, bs = 8, 3, 128
    fe = {"non_linearity": "sigmoid", "stop_epoch": 4, "structural_wt": 0.3}
    ck = str(tmp_path / "ck")

    def new(dist=None, **kw):
        m = ScoringBasedEmbeddingModel(eta=eta, k=k, scoring_type="DistMult", seed=4)
        m._dist_override = dist
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="nll", entity_relation_regularizer="l2", **kw)
        return m

    def body(dist):
        m = new(dist, entity_sharding="rows", sharded_negatives="global")
        h = m.fit(Xw, batch_size=bs, epochs=2, verbose=False, focusE=True, focusE_params=dict(fe))
        m.save_weights(ck)
        h2 = m.fit(Xw, batch_size=bs, epochs=4, initial_epoch=2, verbose=False, focusE=True, focusE_params=dict(fe))
        m.calibrate(X[:200], positive_base_rate=0.4, batch_size=64, epochs=3)
        r_sub = m.evaluate(Xtest, use_filter={"train": X}, corrupt_side="s,o", entities_subset=subset, verbose=False)
        ents = np.array([f"e{i}" for i in range(50)])
        out = (h.history["loss"] + h2.history["loss"], m.get_embeddings(ents), m.predict_proba(Xtest), r_sub)
        # resume from the shard files on 2 ranks
        m2 = new(dist, entity_sharding="rows", sharded_negatives="global")
        m2.load_weights(ck)
        h3 = m2.fit(Xw, batch_size=bs, epochs=4, initial_epoch=2, verbose=False, focusE=True, focusE_params=dict(fe))
        return out + (h3.history["loss"], m2.get_embeddings(ents))

    res = ThreadedWorld(2).run(body)
    assert os.path.exists(ck + ".shard000-of-002.npz") and os.path.exists(ck + ".shard001-of-002.npz")
    assert "ent" not in np.load(ck + ".npz").files
    ents = np.array([f"e{i}" for i in range(50)])
    m1 = new()
    h1 = m1.fit(Xw, batch_size=bs, epochs=4, verbose=False, focusE=True, focusE_params=dict(fe))
    m1.calibrate(X[:200], positive_base_rate=0.4, batch_size=64, epochs=3)
    e1, pp1 = m1.get_embeddings(ents), m1.predict_proba(Xtest)
    r1 = m1.evaluate(Xtest, use_filter={"train": X}, corrupt_side="s,o", entities_subset=subset, verbose=False)
    for hist, emb, pp, r_sub, hist3, emb3 in res:
        assert np.allclose(hist, h1.history["loss"], rtol=2e-4)
        assert (np.abs(emb - e1) <= 1e-5 + 1e-3 * np.abs(e1)).mean() > 0.995
        assert np.allclose(pp, pp1, rtol=1e-3, atol=1e-4)
        assert (np.abs(r_sub - r1) <= 1).mean() > 0.97 and r_sub.max() <= len(subset) + 1
        # the run resumed from the sharded checkpoint == the uninterrupted sharded run (same schedule, same slots)
        # (ten more Adam steps on the atomic path from bit-equal state: equal up to fp32 arrival order, see tests/margins.py)
        assert within("model/sharded_resume/loss", rel_gap(hist3, hist[2:]), 2e-5)
        assert within("model/sharded_resume/emb_frac_outside", frac_outside(emb3, emb, 1e-3, 1e-5), 0.005)
    assert np.array_equal(res[0][3], res[1][3])
    # the 2-rank shard files resumed by ONE model (rows re-sliced, slots included)
    m3 = new()
    m3.load_weights(ck)
    h3 = m3.fit(Xw, batch_size=bs, epochs=4, initial_epoch=2, verbose=False, focusE=True, focusE_params=dict(fe))
    assert np.allclose(h3.history["loss"], h1.history["loss"][2:], rtol=2e-4)
    assert (np.abs(m3.get_embeddings(ents) - e1) <= 1e-5 + 1e-3 * np.abs(e1)).mean() > 0.995
    # and a whole-table checkpoint resumed by 2 row-sharded ranks
    m4 = new()
    m4.fit(Xw, batch_size=bs, epochs=2, verbose=False, focusE=True, focusE_params=dict(fe))
    ck1 = str(tmp_path / "ck1")
    m4.save_weights(ck1)

    def body2(dist):
        m = new(dist, entity_sharding="rows", sharded_negatives="global")
        m.load_weights(ck1)
        h = m.fit(Xw, batch_size=bs, epochs=4, initial_epoch=2, verbose=False, focusE=True, focusE_params=dict(fe))
        return h.history["loss"], m.get_embeddings(ents)

    for hist, emb in ThreadedWorld(2).run(body2):
        assert np.allclose(hist, h1.history["loss"][2:], rtol=2e-4)
        assert (np.abs(emb - e1) <= 1e-5 + 1e-3 * np.abs(e1)).mean() > 0.995



def test_dp_fit_with_measured_merge_schedule(gpu_lib, monkeypatch):
    """AMDKGE_DP_MERGE=auto: fit() spends the first steps of the first epoch on StepLoop.tune_merge (every candidate schedule
    computes the same update), keeps one, and ends with the tables of the single-GPU fit."""
    from threaded_dist import ThreadedWorld

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers

    X = toy_graph(n=1600, N=60, R=4)
    k, eta, bs, epochs = 8, 3, 64, 2   # 25 steps per epoch: enough for 3 candidates x (1 + 4) steps

    def make(dist=None):
        m = ScoringBasedEmbeddingModel(eta=eta, k=k, scoring_type="ComplEx", seed=2)
        m._dist_override = dist
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="nll")
        m.fit(X, batch_size=bs, epochs=epochs, verbose=False)
        return m

    m1 = make()
    e1, r1 = m1._engine.get_tables()
    monkeypatch.setenv("AMDKGE_DP_MERGE", "auto")

    def body(dist):
        m = make(dist)
        assert m._loop.merge_report is not None and len(m._loop.merge_report) == 3 and not m._loop.auto_tune
        ed, rd = m._engine.get_tables()
        assert np.mean(np.abs(ed - e1) <= 1e-5 + 1e-3 * np.abs(e1)) > 0.995 and np.abs(rd - r1).max() < 2.5e-2
        assert np.allclose(m.history.history["loss"][1], m1.history.history["loss"][1], rtol=2e-4)   # second epoch: all steps
        return float(np.abs(ed).sum())

    a, b = ThreadedWorld(2).run(body)
    assert a == b


def test_optimizer_wrapper_state_access(gpu_lib):
    """The reference's structural optimizer tests (tests/ampligraph/latent_features/test_optimizers.py:16-84): weights list =
    iterations + state tensors x (entity, relation), get/set round trip, iteration count, entity / relation accessors."""
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers

    X = toy_graph(7)
    for name, n_state in (("adam", 2), ("adagrad", 1), ("sgd", 0)):
        opt = optimizers.get(name)
        opt.set_partitioned_training()
        m = ScoringBasedEmbeddingModel(eta=2, k=5, scoring_type="DistMult", seed=0)
        m.compile(optimizer=opt, loss="nll")
        m.fit(X[:100], batch_size=100, epochs=1, verbose=False)
        w = opt.get_weights()
        assert len(w) == 1 + opt.get_hyperparam_count() * opt.num_optimized_vars and opt.get_hyperparam_count() == n_state
        assert opt.get_iterations() == 1
        opt.set_weights(w)
        assert all(np.all(a == b) for a, b in zip(w, opt.get_weights()))
        ent_h, rel_h = opt.get_entity_relation_hyperparams()
        assert len(ent_h) == len(rel_h) == n_state
        if n_state == 2:
            assert (w[1] == ent_h[0]).all() and (w[3] == ent_h[1]).all() and (w[2] == rel_h[0]).all() and (w[4] == rel_h[1]).all()
            assert w[1].shape == (m._n_ents, 5) and w[2].shape == (m._n_rels, 5) and np.abs(w[1]).max() > 0
            opt.set_entity_relation_hyperparams([np.zeros_like(ent_h[0]), ent_h[1]], rel_h)
            assert np.abs(opt.get_weights()[1]).max() == 0 and (opt.get_weights()[3] == w[3]).all()


def test_save_model_restore_model_roundtrip(gpu_lib, tmp_path):
    """ampligraph.utils.save_model / restore_model (utils/model_utils.py:29-129) on the engine's own format: same predictions
    and ranks after the round trip, optimizer state and regulariser restored (continued training == uninterrupted), config."""
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers, regularizers
    from ampligraph_amd.utils import restore_model, save_model

    X = toy_graph(9, n=600)

    def make():
        m = ScoringBasedEmbeddingModel(eta=3, k=6, scoring_type="ComplEx", seed=2)
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="self_adversarial",
                  entity_relation_regularizer=regularizers.get("LP", {"p": 3, "lambda": 1e-3}))
        return m

    full = make()
    h_full = full.fit(X, batch_size=200, epochs=4, verbose=False)
    m = make()
    m.fit(X, batch_size=200, epochs=2, verbose=False)
    path = str(tmp_path / "saved_model")
    save_model(m, path)
    save_model(m, path)                       # an existing path is overwritten
    m.save(str(tmp_path / "saved_via_method"))
    r = restore_model(path)
    assert r.get_config() == m.get_config() and ScoringBasedEmbeddingModel.from_config(m.get_config()).k == 6
    assert np.array_equal(r.predict(X[:50]), m.predict(X[:50]))
    assert np.array_equal(r.evaluate(X[:40], use_filter={"train": X}, verbose=False), m.evaluate(X[:40], use_filter={"train": X}, verbose=False))
    assert r.optimizer.iterations == m.optimizer.iterations and r._regularizers[0].p == 3
    h = r.fit(X, batch_size=200, epochs=4, initial_epoch=2, verbose=False)
    assert np.allclose(h.history["loss"], h_full.history["loss"][2:], rtol=1e-4)
    s, p, o = r.get_invalid_keys(np.array([["e1", "r0", "nope"], ["zzz", "r9", "e2"]]))
    assert list(s) == ["zzz"] and list(p) == ["r9"] and list(o) == ["nope"]
    with pytest.raises(FileNotFoundError):
        restore_model(str(tmp_path / "missing"))
