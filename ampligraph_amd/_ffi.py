"""ctypes binding of libamdkge.so (C ABI declared in include/amdkge.h).

The library is the product: there is no CPU fallback.  `lib()` raises `AmdKgeLibraryError` when the
shared object is missing or does not export the ABI version this package was written for.
"""
import ctypes as C
import os

# torch bundles its own HIP runtime (soname libamdhip64.so.7, same soname as /opt/rocm's).  It must be
# the first one mapped into the process so that libamdkge and torch share ONE runtime (one set of
# devices, streams and allocations); loading libamdkge first would pull /opt/rocm's copy and leave
# the process with mismatched HIP/HSA runtimes.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AMDKGE_LIB") or os.path.join(_HERE, "lib", "libamdkge.so")   # AMDKGE_LIB: development builds
ABI_VERSION = 5

# error classes (the return values of the entry points), enums and flag bits of include/amdkge.h
OK, EINVAL, EHIP, ERCCL, ENOMEM, EUNSUPPORTED = 0, -1, -2, -3, -4, -5
SCORING_TYPES = {"TransE": 0, "DistMult": 1, "ComplEx": 2, "HolE": 3, "RotatE": 4}
LOSSES = {"pairwise": 0, "nll": 1, "absolute_margin": 2, "self_adversarial": 3, "multiclass_nll": 4}
OPTIMIZERS = {"sgd": 0, "adagrad": 1, "adam": 2, "momentum": 3, "rmsprop": 4, "rmsprop_mom": 5, "adadelta": 6, "adamax": 7}
# optimizer state tensors per table, in the slot order of include/amdkge.h (checkpoint keys are "<name>_e" / "<name>_r")
OPT_SLOTS = {"sgd": (), "adagrad": ("a",), "adam": ("m", "v"), "momentum": ("mom",), "rmsprop": ("rms",),
             "rmsprop_mom": ("rms", "mom"), "adadelta": ("acc", "dacc"), "adamax": ("m", "u")}
SIDE_S, SIDE_O = 1, 2
RANK_STRATEGY = {"worst": 0, "best": 1, "middle": 2}
FOCUS_NONLINEARITY = {"linear": 1, "tanh": 2, "sigmoid": 3, "softplus": 4}
# AMDKGE_TILED_*: the flags of amdkge_train_step_tiled / amdkge_train_tiled_status, and what amdkge_session_config.flags holds
TILED_POS_ATOMIC, TILED_DETERMINISTIC, TILED_HOT_ROWS, TILED_GIVEN_COEFFS, TILED_DET_WIDE_SORT = 1, 2, 4, 8, 16
# AMDKGE_GROUP_*: the flags of amdkge_session_group_create_ex / _rows / _cols (ROWS and COLS are set by the library)
GROUP_FORCE_RCCL, GROUP_ROWS, GROUP_GLOBAL_NEGATIVES, GROUP_COLS, GROUP_FORCE_THREADS = 1, 2, 4, 8, 16
NEG_SIDE_MODES = {"uniform": 0, "bernoulli": 1, "s": 2, "o": 3}   # AMDKGE_NEG_SIDE_*, include/amdkge_negatives.h; amdkge_shared.h uses them too
NEG_MAX_TRIES = 32
SHARED_MAX_NEGS = (1 << 24) - 1                  # include/amdkge_shared.h
SHARED_LIST_MODES = {"given": 0, "identity": 1}  # AMDKGE_SHARED_LIST_*, include/amdkge_shared_mask.h
BATCH_REG_NORMS = {"float": 0, "modulus": 1}     # AMDKGE_BATCH_REG_*, include/amdkge_batch_reg.h


class AmdKgeLibraryError(RuntimeError):
    pass


class AmdKgeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libamdkge error {code}: {msg}")
        self.code = code


class Model(C.Structure):
    _fields_ = [("scoring_type", C.c_int32), ("k", C.c_int32), ("n_ents", C.c_int64), ("n_rels", C.c_int64),
                ("max_rel_size", C.c_int32), ("k_pad", C.c_int32), ("k_full", C.c_int32), ("reserved_", C.c_int32)]


class Loss(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reduction_mean", C.c_int32), ("margin", C.c_float), ("alpha", C.c_float),
                ("focus_nonlinearity", C.c_int32), ("focus_beta", C.c_float), ("d_focus_w", C.c_void_p)]


class Opt(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reg_p", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("epsilon", C.c_float), ("reg_lambda", C.c_float), ("iteration", C.c_int64),
                ("lazy", C.c_int32), ("row_floats", C.c_int32),
                # ABI 3: second LP term of the swept table; the relation table's terms where one call sweeps both
                ("reg2_p", C.c_int32), ("reg2_lambda", C.c_float), ("rel_reg_p", C.c_int32), ("rel_reg2_p", C.c_int32),
                ("rel_reg2_lambda", C.c_float)]


class SessionConfig(C.Structure):
    _fields_ = [("model", Model), ("loss", Loss), ("opt", Opt), ("rel_reg_lambda", C.c_float), ("eta", C.c_int32),
                ("seed", C.c_uint64), ("device", C.c_int32), ("flags", C.c_int32)]


TABLES = {"ent": 0, "rel": 1, "ent_slot0": 2, "ent_slot1": 3, "rel_slot0": 4, "rel_slot1": 5}
CORRUPT_SIDES = {"s": 1, "o": 2, "s,o": 3, "s+o": 4}

P = C.c_void_p
I64 = C.c_int64
I32 = C.c_int32
U64 = C.c_uint64

# ABI: header -> {name: (restype, argtypes)}, every entry point the headers under include/ declare, the headers in the order they were
# added.  This table is what lib() binds -- the package does not read include/ -- and tests/test_abi_host.py holds it, the four
# Structures above and every constant of this module equal to the headers.  A new extension header is one more entry here.
ABI = {}
ABI["amdkge.h"] = {   # the frozen declaration set of ABI 5
    "amdkge_abi_version": (C.c_int, []),
    "amdkge_release_scratch": (C.c_int, []),
    "amdkge_set_rank_early": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "amdkge_last_error": (C.c_char_p, []),
    "amdkge_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "amdkge_set_device": (C.c_int, [C.c_int]),
    "amdkge_dev_alloc": (C.c_int, [C.POINTER(P), U64]),
    "amdkge_dev_free": (C.c_int, [P]),
    "amdkge_h2d": (C.c_int, [P, P, U64, P]),
    "amdkge_d2h": (C.c_int, [P, P, U64, P]),
    "amdkge_dev_memset": (C.c_int, [P, C.c_int, U64, P]),
    "amdkge_stream_sync": (C.c_int, [P]),
    "amdkge_internal_k": (C.c_int, [C.c_int, C.c_int]),
    "amdkge_padded_k": (C.c_int, [C.c_int]),
    "amdkge_row_floats": (C.c_int, [C.POINTER(Model)]),
    "amdkge_pack_rows": (C.c_int, [C.POINTER(Model), P, I64, P, P]),
    "amdkge_unpack_rows": (C.c_int, [C.POINTER(Model), P, I64, P, P]),
    "amdkge_set_rank_kernel": (C.c_int, [C.c_int]),
    "amdkge_set_rank_rotate_fast": (C.c_int, [C.c_int]),
    "amdkge_rank_screen_workspace_bytes": (I64, [C.POINTER(Model), I64, I64]),
    "amdkge_rank_counts_screened": (C.c_int, [C.POINTER(Model), P, P, P, I64, I32, P, I64, I64, P, P, P, I64, P]),
    "amdkge_set_tile_direct": (C.c_int, [C.c_int]),
    "amdkge_filter_build_workspace_bytes": (I64, [I64, I64, I64]),
    "amdkge_filter_build": (C.c_int, [P, I64, I32, I64, I64, P, P, P, P, P, P]),
    "amdkge_score": (C.c_int, [C.POINTER(Model), P, P, P, I64, P, P]),
    "amdkge_platt_step": (C.c_int, [P, I64, P, I64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, P, P]),
    "amdkge_sample_corruptions": (C.c_int, [P, I64, I32, I64, I64, U64, U64, I64, I64, P, P]),
    "amdkge_train_fwdbwd": (C.c_int, [C.POINTER(Model), C.POINTER(Loss), P, P, P, I64, I32, I64, I64, U64, U64,
                                      I64, I64, P, P, P, P, P, P, P]),
    "amdkge_opt_step": (C.c_int, [C.POINTER(Opt), P, P, P, P, I64, P, P]),
    "amdkge_cols_partial_scores": (C.c_int, [C.POINTER(Model), P, P, P, I64, I32, I64, I64, U64, U64, I64, I64, P, P, P]),
    "amdkge_cols_loss": (C.c_int, [C.POINTER(Model), C.POINTER(Loss), P, I64, I32, P, P]),
    "amdkge_train_tiled_workspace_bytes": (I64, [C.POINTER(Model), I64, I32]),
    "amdkge_train_step_tiled": (C.c_int, [C.POINTER(Model), C.POINTER(Loss), C.POINTER(Opt), P, P, P, P, P, P, C.c_float,
                                          P, I64, I32,
                                          I64, I64, U64, U64, I64, I64, P, P, P, I32, I32, P, P, P, P, P, P]),
    "amdkge_train_tiled_set_hot_rows": (C.c_int, [C.POINTER(Model), P, P, I32, P]),
    "amdkge_train_tiled_status": (C.c_int, [C.POINTER(Model), I64, I32, I32, P, C.POINTER(C.c_int32), P]),
    "amdkge_rank_workspace_bytes": (I64, [C.POINTER(Model), I64]),
    "amdkge_rank_counts": (C.c_int, [C.POINTER(Model), P, P, P, I64, I32, P, I64, I64, P, P, P]),
    "amdkge_rank_filter": (C.c_int, [C.POINTER(Model), P, P, P, I64, I32, P, P, P, P, I64, I64, P, P, P]),
    "amdkge_rank_compose": (C.c_int, [P, P, I64, I32, P, I64, P]),
    "amdkge_filter_ranges": (C.c_int, [P, P, I64, P, I64, I32, I64, I64, P, P, P]),
    "amdkge_corruption_scores": (C.c_int, [C.POINTER(Model), P, P, P, I64, I32, P, I64, I64, P, I64, P, P]),
    "amdkge_row_dots": (C.c_int, [P, I64, P, I32, P, I64, I64, P, I64, P]),
    "amdkge_row_sqnorms": (C.c_int, [P, I32, P, I64, I64, C.c_float, I32, P, P]),
    "amdkge_pair_distances": (C.c_int, [P, I64, P, I32, P, I64, P, I32, I32, P, P]),
    "amdkge_topk_rows": (C.c_int, [P, I64, I64, I64, P, P, P, I32, I32, P, P, P]),
    "amdkge_topk_rows_excluding": (C.c_int, [P, I64, I64, I64, P, I64, P, P, P, P, I32, P, P, P]),
    "amdkge_relation_workspace_bytes": (I64, [C.POINTER(Model), I64]),
    "amdkge_relation_scores": (C.c_int, [C.POINTER(Model), P, P, P, I64, P, I64, I64, P, I64, P, P]),
    "amdkge_relation_rank_counts": (C.c_int, [P, I64, I64, I64, P, P, I64, P, P, P, P, P, P, P]),
    "amdkge_pair_filter_build": (C.c_int, [P, I64, I64, I64, P, P, P, P, P, P]),
    "amdkge_pair_filter_ranges": (C.c_int, [P, P, I64, P, I64, I64, P, P, P]),
    "amdkge_discover_select": (C.c_int, [P, I64, I64, I64, P, I32, P, P, P, I32, I32, P, I32, I64, P, I64, P, P]),
    "amdkge_join_nearest": (C.c_int, [P, I64, I32, P, P, P, P, P]),
    "amdkge_join_radius": (C.c_int, [P, I64, I32, C.c_double, P, I64, P, P]),
    "amdkge_join_dbscan_workspace_bytes": (I64, [I64]),
    "amdkge_join_dbscan": (C.c_int, [P, I64, I32, C.c_double, I32, P, P, P, P, P]),
    "amdkge_kmeans_workspace_bytes": (I64, [I64, I32, I32, I32]),
    "amdkge_kmeans_assign": (C.c_int, [P, I64, I32, P, I32, I32, P, P, P]),
    "amdkge_kmeans_lloyd": (C.c_int, [P, I64, I32, P, I32, I32, I32, C.c_double, P, P, P, P, P, P]),
    "amdkge_shard_route_workspace_bytes": (I64, [I64, I64]),
    "amdkge_shard_route": (C.c_int, [I64, I32, I32, P, I64, P, I64, I32, P, P, P, P, P, P]),
    "amdkge_gather_rows": (C.c_int, [P, I32, P, I64, P, P]),
    "amdkge_scatter_add_rows": (C.c_int, [P, I32, P, I64, P, P]),
    "amdkge_opt_step_merged": (C.c_int, [C.POINTER(Opt), P, P, I32, I64, P, P, I64, P, P]),
    "amdkge_synth_triples": (C.c_int, [U64, I64, I64, I64, I64, P, P]),
    "amdkge_session_create": (C.c_int, [C.POINTER(SessionConfig), C.POINTER(P)]),
    "amdkge_session_destroy": (None, [P]),
    "amdkge_session_set_rows": (C.c_int, [P, I32, I64, I64, P]),
    "amdkge_session_get_rows": (C.c_int, [P, I32, P, I64, I64, P]),
    "amdkge_session_train_step": (C.c_int, [P, P, I64, P, C.POINTER(C.c_double)]),
    "amdkge_session_set_hot_rows": (C.c_int, [P, P, I32]),
    "amdkge_session_score": (C.c_int, [P, P, I64, P]),
    "amdkge_session_rank": (C.c_int, [P, P, I64, P, P, P, P, P, I64, I32, I32, P]),
    "amdkge_session_group_create": (C.c_int, [C.POINTER(SessionConfig), P, I32, C.POINTER(C.c_void_p)]),
    "amdkge_session_group_create_ex": (C.c_int, [C.POINTER(SessionConfig), P, I32, I32, C.POINTER(C.c_void_p)]),
    "amdkge_session_group_info": (C.c_int, [P, C.POINTER(I32), C.POINTER(I32)]),
    "amdkge_session_group_create_rows": (C.c_int, [C.POINTER(SessionConfig), P, I32, I32, I64, C.POINTER(C.c_void_p)]),
    "amdkge_session_group_create_cols": (C.c_int, [C.POINTER(SessionConfig), P, I32, I32, C.POINTER(C.c_void_p)]),
    "amdkge_session_group_get_rows": (C.c_int, [P, I32, P, I64, I64, P]),
    "amdkge_session_group_route_overflow": (C.c_int, [P, C.POINTER(I32)]),
    "amdkge_session_screen_stats": (C.c_int, [P, C.POINTER(I32), C.POINTER(I64), C.POINTER(I32)]),
    "amdkge_session_group_destroy": (None, [P]),
    "amdkge_session_group_size": (I32, [P]),
    "amdkge_session_group_replica": (C.c_int, [P, I32, C.POINTER(C.c_void_p)]),
    "amdkge_session_group_set_rows": (C.c_int, [P, I32, I64, I64, P]),
    "amdkge_session_group_train_step": (C.c_int, [P, P, I64, P, C.POINTER(C.c_double)]),
    "amdkge_session_group_rank": (C.c_int, [P, P, I64, P, P, P, P, P, I64, I32, I32, P]),
}

ABI["amdkge_lists.h"] = {   # ranking against per-triple candidate lists
    "amdkge_rank_lists_workspace_bytes": (I64, [C.POINTER(Model), I64]),
    "amdkge_rank_lists": (C.c_int, [C.POINTER(Model), P, P, I64, P, I64, I32, P, P, P, I64, P, P, P, P, P, P, P, P]),
}

ABI["amdkge_negatives.h"] = {   # training negative samplers
    "amdkge_sample_negatives": (C.c_int, [P, I64, I32, I64, I64, U64, U64, I64, I64, I32, P, P, I64, P, P, P, P, P, P, I32, P, P, P]),
    "amdkge_negatives_side_thresholds": (C.c_int, [P, I64, P, I64, I64, I64, P, P]),
}

ABI["amdkge_shared.h"] = {   # shared-negative training
    "amdkge_sample_shared": (C.c_int, [P, I64, I64, I32, I64, I64, U64, U64, I32, P, P, I64, P, P, P]),
    "amdkge_train_shared_workspace_bytes": (I64, [C.POINTER(Model), I64, I64, I32]),
    "amdkge_train_shared_fwdbwd": (C.c_int, [C.POINTER(Model), C.POINTER(Loss), P, P, P, I64, I64, I32, P, P, P, P, P, P, P, P, P]),
}

ABI["amdkge_types.h"] = {   # type-constrained negatives and evaluation: per-relation domain / range sets
    "amdkge_relation_sets_build": (C.c_int, [P, I64, I32, I64, I64, P, P, P, P, P, P]),
    "amdkge_relation_sets_ranges": (C.c_int, [P, P, I64, P, I64, I64, I64, I64, P, P, P]),
    "amdkge_sample_negatives_typed": (C.c_int, [P, I64, I32, I64, I64, U64, U64, I64, I64, I32, P, P, I64, P, P, P, P, P, P, I32, P, P,
                                                P, P, P, P, P, P, P]),
}

ABI["amdkge_shared_mask.h"] = {   # shared negatives with known statements masked; the all-entities list
    "amdkge_shared_mask_scores": (C.c_int, [P, I64, I64, I64, I32, P, P, P, P, P, P, P, P, I32, P, P]),
    "amdkge_train_shared_masked_fwdbwd": (C.c_int, [C.POINTER(Model), C.POINTER(Loss), P, P, P, I64, I64, I32, P, P, P, P, P, P, P, P,
                                                    P, P, P, P, P, P, I32, P, P]),
}

ABI["amdkge_shared_dist.h"] = {   # shared negatives for the distance models, TransE and RotatE, on distance tiles
    "amdkge_train_shared_dist_workspace_bytes": (I64, [C.POINTER(Model), I64, I64, I32]),
    "amdkge_train_shared_dist_fwdbwd": (C.c_int, [C.POINTER(Model), C.POINTER(Loss), P, P, P, I64, I64, I32, P, P, P, P, P, P, P, P,
                                                  P, P, P, P, P, P, I32, P, P]),
}

ABI["amdkge_batch_reg.h"] = {   # batch regularisers: N3 and per-occurrence Lp on the rows of a step's positives
    "amdkge_batch_reg_fwdbwd": (C.c_int, [C.POINTER(Model), P, P, P, I64, I32, C.c_float, I32, I32, C.c_float, I32, P, P, P, P]),
}

ABI["amdkge_shared_labels.h"] = {   # KvsAll on the shared step: binary cross-entropy with multi-hot labels
    "amdkge_shared_label_loss": (C.c_int, [P, I64, I64, I64, I32, P, P, P, P, P, P, P, P, I32, C.c_float, I32, C.c_float, P, P, P, P, P]),
    "amdkge_train_shared_labels_fwdbwd": (C.c_int, [C.POINTER(Model), C.c_float, I32, P, P, P, I64, I64, I32, P, P, P, P, P, P, P, P,
                                                    P, P, P, P, P, P, I32, P, P, P, P]),
    "amdkge_train_shared_dist_labels_fwdbwd": (C.c_int, [C.POINTER(Model), C.c_float, I32, P, P, P, I64, I64, I32, P, P, P, P, P, P, P, P,
                                                         P, P, P, P, P, P, I32, P, P, P, P]),
}

ABI["amdkge_relation_objective.h"] = {   # the relation-prediction training objective: a softmax over the relation table
    "amdkge_train_relation_workspace_bytes": (I64, [C.POINTER(Model), I64]),
    "amdkge_train_relation_fwdbwd": (C.c_int, [C.POINTER(Model), C.POINTER(Loss), C.c_float, P, P, P, I64, P, P, P, P, P, P, P, P, P, P, P]),
}

# ABI_EXT: the same table for the headers under include/ext/.  There are two tables because ABI is held, name for name and header for
# header, to the closed set of headers directly under include/ (tests/test_abi_host.py); what is added behind that set is declared one
# directory down and listed here (tests/test_abi_ext_host.py holds it to its headers by the same rules).
ABI_EXT = {}
ABI_EXT["ext/amdkge_sparse.h"] = {   # sparse optimizer mode: a step's candidate rows and the sweep of a list of rows
    "amdkge_step_rows_workspace_bytes": (I64, [I64, I64]),
    "amdkge_step_rows": (C.c_int, [I64, P, I64, P, I64, P, I64, P, P, P]),
    "amdkge_opt_step_rows": (C.c_int, [C.POINTER(Opt), P, P, P, P, I64, P, P, I64, P, P]),
}

_lib = None


def lib():
    """Load (once) and return the bound library; raise loudly if it cannot be used."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmdKgeLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C ampligraph_amd/csrc`). ampligraph_amd has no CPU fallback.")
    try:
        handle = C.CDLL(LIB_PATH)
    except OSError as e:  # missing libamdhip64 etc.
        raise AmdKgeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in [entry for table in list(ABI.values()) + list(ABI_EXT.values()) for entry in table.items()]:
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise AmdKgeLibraryError(f"{LIB_PATH} does not export {name}; stale build?") from e
        fn.restype = res
        fn.argtypes = args
    if handle.amdkge_abi_version() != ABI_VERSION:
        raise AmdKgeLibraryError("libamdkge ABI version mismatch; rebuild the library")
    _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        raise AmdKgeError(rc, lib().amdkge_last_error().decode("utf-8", "replace"))
