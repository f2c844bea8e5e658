"""numpy restatement of include/amdkge_batch_reg.h (batch regularisers: N3 and per-occurrence Lp on the rows of a step's positives):
test infrastructure, the product does not import it.

Tables are DENSE rows [n, NC * k] ([re || im] halves for the complex models).  Every per-unit value is rounded to fp32 where the
header's operation order rounds it (m2 = fl(fl(re re) + fl(im im)), m = fl(sqrt(m2)), pen = m2 | fl(m2 m), c = fl(p lambda),
f = c | fl(c m), g = fl(f x)); every SUM -- a row's penalty over its units, the batch's penalty over its positives, a gradient row
over the row's occurrences -- is taken in fp64, which is what the kernel's fp32 lane sums, double accumulator and unordered fp32
atomics are held against (penalty 1e-6 relative, gradients 1e-5 of the row's largest magnitude).

penalty_torch is the same penalty as a differentiable float64 torch expression (no rounding to fp32): the CPU tests hold the
restatement's gradient to its autograd gradient."""
import numpy as np

F32 = np.float32
FLOAT, MODULUS = 0, 1
NORMS = {"float": FLOAT, "modulus": MODULUS}
COMPLEX = ("ComplEx", "HolE", "RotatE")
MODELS = ("TransE", "DistMult", "ComplEx", "HolE", "RotatE")


def nc_of(model):
    return 2 if model in COMPLEX else 1


def modulus_allowed(model, table):
    """the header's rule: ComplEx / HolE both tables, RotatE the entity table only ("ent" | "rel")"""
    return model in ("ComplEx", "HolE") or (model == "RotatE" and table == "ent")


def norms_of(model):
    """[(norm_ent, norm_rel), ...]: every combination of norm modes the header allows for `model`"""
    return [(ne, nr) for ne in ((FLOAT, MODULUS) if modulus_allowed(model, "ent") else (FLOAT,))
            for nr in ((FLOAT, MODULUS) if modulus_allowed(model, "rel") else (FLOAT,))]


def row_terms(rows, k, nc, p, lam, norm):
    """rows fp32 [n, nc * k] -> (pen float64 [n]: sum_u n^p of each row, WITHOUT lambda; grad fp32 [n, nc * k]: the gradient ONE
    occurrence of the row adds)"""
    assert p in (2, 3) and norm in (FLOAT, MODULUS) and (norm == FLOAT or nc == 2)
    rows = np.ascontiguousarray(rows, dtype=F32)
    c = F32(F32(p) * F32(lam))
    with np.errstate(all="ignore"):
        if norm == MODULUS:
            re, im = rows[:, :k], rows[:, k:]
            m2 = (re * re).astype(F32) + (im * im).astype(F32)
            m = np.sqrt(m2).astype(F32)
            pen = m2 if p == 2 else (m2 * m).astype(F32)
            f = np.broadcast_to(c, m.shape) if p == 2 else (c * m).astype(F32)
            grad = np.concatenate([(f * re).astype(F32), (f * im).astype(F32)], 1)
        else:
            a, n = (rows * rows).astype(F32), np.abs(rows)
            pen = a if p == 2 else (a * n).astype(F32)
            grad = (c * rows).astype(F32) if p == 2 else ((c * n).astype(F32) * rows).astype(F32)
        return pen.astype(np.float64).sum(1), grad


def batch_reg(model, k, ent, rel, X, p_e, lam_e, norm_e, p_r, lam_r, norm_r):
    """-> (R float64; G_ent float64 [N, NC * k]; G_rel float64 [n_rels, NC * k]): the penalty of the batch X int [B, 3] and what the
    call adds to zeroed gradient tables.  A row is counted once per occurrence (s and o of one positive are two occurrences)."""
    nc = nc_of(model)
    ent, rel, X = np.asarray(ent, F32), np.asarray(rel, F32), np.asarray(X, np.int64).reshape(-1, 3)
    Ge, Gr = np.zeros(ent.shape, np.float64), np.zeros(rel.shape, np.float64)
    R = 0.0
    with np.errstate(all="ignore"):
        if float(lam_e) != 0.0:
            occ = np.concatenate([X[:, 0], X[:, 2]])
            pen, grad = row_terms(ent[occ], k, nc, p_e, lam_e, norm_e)
            R += float(F32(lam_e)) * float(pen.sum())
            np.add.at(Ge, occ, grad.astype(np.float64))
        if float(lam_r) != 0.0:
            pen, grad = row_terms(rel[X[:, 1]], k, nc, p_r, lam_r, norm_r)
            R += float(F32(lam_r)) * float(pen.sum())
            np.add.at(Gr, X[:, 1], grad.astype(np.float64))
    return R, Ge, Gr


def penalty_torch(model, k, ent, rel, X, p_e, lam_e, norm_e, p_r, lam_r, norm_r):
    """the same penalty of float64 torch tables, differentiable; powers are written so that a unit at exactly zero has gradient zero
    ((re^2 + im^2)^(3/2) and |x|^3, never a square root on its own)"""
    import torch

    X = torch.as_tensor(np.asarray(X, np.int64).reshape(-1, 3))

    def term(rows, p, norm):
        if norm == MODULUS:
            m2 = rows[:, :k] ** 2 + rows[:, k:] ** 2
            return (m2 if p == 2 else m2 ** 1.5).sum()
        return (rows ** 2 if p == 2 else rows.abs() ** 3).sum()

    R = torch.zeros((), dtype=torch.float64)
    if float(lam_e) != 0.0:
        R = R + float(F32(lam_e)) * (term(ent[X[:, 0]], p_e, norm_e) + term(ent[X[:, 2]], p_e, norm_e))
    if float(lam_r) != 0.0:
        R = R + float(F32(lam_r)) * term(rel[X[:, 1]], p_r, norm_r)
    return R


def tables(model, k, N, R, seed=0, scale=0.3):
    rng = np.random.default_rng(seed)
    nc = nc_of(model)
    return (rng.normal(size=(N, nc * k)) * scale).astype(F32), (rng.normal(size=(R, nc * k)) * scale).astype(F32)


def triples(rng, B, N, R):
    return np.stack([rng.integers(0, N, B), rng.integers(0, R, B), rng.integers(0, N, B)], 1).astype(np.int32)


def assert_rows_close(G, T, tol=1e-5):
    """the project's default-mode bar: every float within tol of its ROW's largest reference magnitude (the order of the atomic adds
    is free).  A row whose reference is all zero must be all zero."""
    T = np.asarray(T, np.float64)
    G = np.asarray(G, np.float64)
    scale = np.abs(T).max(axis=1, keepdims=True)
    zero = scale[:, 0] == 0.0
    assert not G[zero].any(), "a row nothing was added to is not zero"
    err = np.abs(G - T)[~zero] / scale[~zero]
    assert err.size == 0 or err.max() <= tol, err.max()
