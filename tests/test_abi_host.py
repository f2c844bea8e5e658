"""ampligraph_amd/_ffi.py against the headers under include/, without a GPU: every entry point's name, return type and argument list
(count, order, types) as the header declares them (tests/abi_decl.py parses and maps them) and as lib() bound them; the four Structures
and every constant against what the C compiler makes of the headers (a small host program of its own: sizeof, offsetof, values).  A new
extension header needs no new text here, unless it brings constants (twins / UNUSED) or must stay unknown to an older one (UNKNOWN_TO)."""
import ctypes as C
import subprocess

import pytest

import abi_decl as D
from ampligraph_amd import _ffi

# older header -> words of later headers it must not contain: the frozen headers were not touched when those were added
UNKNOWN_TO = {"amdkge.h": ("amdkge_shared", "shared_dist", "amdkge_relation_objective"),
              "amdkge_shared.h": ("amdkge_shared_mask", "shared_dist"), "amdkge_shared_mask.h": ("shared_dist",)}
# header constants without a Python twin, and why the Python side does not use them
UNUSED = {"AMDKGE_FOCUS_OFF": "0 is Loss.focus_nonlinearity's zero-initialised default; FOCUS_NONLINEARITY names only the modes that are on"}
# the tables of _ffi whose keys are not the header's spelling in lower case
CORRUPT, NEG_SIDE = {"s": "S", "o": "O", "s,o": "S_O", "s+o": "S_PLUS_O"}, {"uniform": "UNIFORM", "bernoulli": "BERNOULLI", "s": "S_ONLY", "o": "O_ONLY"}


def twins():
    """header constant -> the value _ffi holds for it"""
    pairs = [("AMDKGE_" + name, getattr(_ffi, name)) for name in (
        "ABI_VERSION", "OK", "EINVAL", "EHIP", "ERCCL", "ENOMEM", "EUNSUPPORTED", "SIDE_S", "SIDE_O", "NEG_MAX_TRIES", "SHARED_MAX_NEGS",
        "TILED_POS_ATOMIC", "TILED_DETERMINISTIC", "TILED_HOT_ROWS", "TILED_GIVEN_COEFFS", "TILED_DET_WIDE_SORT",
        "GROUP_FORCE_RCCL", "GROUP_ROWS", "GROUP_GLOBAL_NEGATIVES", "GROUP_COLS", "GROUP_FORCE_THREADS")]
    for prefix, table, spell in (("", _ffi.SCORING_TYPES, {}), ("LOSS_", _ffi.LOSSES, {}), ("OPT_", _ffi.OPTIMIZERS, {}), ("RANK_", _ffi.RANK_STRATEGY, {}),
                                 ("FOCUS_", _ffi.FOCUS_NONLINEARITY, {}), ("TABLE_", _ffi.TABLES, {}), ("SHARED_LIST_", _ffi.SHARED_LIST_MODES, {}),
                                 ("BATCH_REG_", _ffi.BATCH_REG_NORMS, {}), ("CORRUPT_", _ffi.CORRUPT_SIDES, CORRUPT), ("NEG_SIDE_", _ffi.NEG_SIDE_MODES, NEG_SIDE)):
        pairs += [("AMDKGE_" + prefix + spell.get(key, key.upper()), value) for key, value in table.items()]
    assert len(dict(pairs)) == len(pairs)
    return dict(pairs)


def test_the_table_names_every_header_and_every_name_once():
    assert set(_ffi.ABI) == set(D.HEADERS) and list(_ffi.ABI)[0] == "amdkge.h"
    names = [n for table in _ffi.ABI.values() for n in table]
    assert len(names) == len(set(names)) == 107
    assert not [(older, w) for older, words in UNKNOWN_TO.items() for w in words if w in D.text(older)]


@pytest.mark.parametrize("header", list(_ffi.ABI))
def test_names_and_types_are_the_headers(header):
    """the loose and the parsed names are the table's; each declaration maps to the table's entry under abi_decl's rule, and so is it bound"""
    table, decls = _ffi.ABI[header], D.declarations(header)
    assert D.declared_names(header) == set(decls) == set(table), D.declared_names(header) ^ set(table)
    for name, (res, params) in decls.items():
        want_res, want_args = table[name]
        assert D.matches(res, want_res, _ffi), f"{name}: returns {res}, the table says {want_res}"
        assert len(params) == len(want_args), f"{name}: {len(params)} parameters declared, {len(want_args)} in the table"
        for i, ((c_type, pname), ct) in enumerate(zip(params, want_args)):
            assert D.matches(c_type, ct, _ffi), f"{name}: parameter {i} is `{c_type} {pname}`, the table says {ct.__name__}"
        fn = getattr(_ffi.lib(), name)
        assert fn.restype is want_res and list(fn.argtypes) == list(want_args), name


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """what the C compiler makes of the headers: (struct_fields, constant_names, {"S name": size, "F struct field": (offset, size), "C name": value})"""
    structs = {s: f for h in D.HEADERS for s, f in D.struct_fields(h).items()}
    consts = [c for h in D.HEADERS for c in D.constant_names(h)]
    assert set(structs) == set(D.STRUCTS) and len(consts) == len(set(consts)) > 60
    lines = ["#include <stddef.h>", "#include <stdio.h>"] + [f'#include "{h}"' for h in D.HEADERS] + ["int main(void) {"]
    for s, fields in structs.items():
        lines.append(f'    printf("S {s} %lu\\n", (unsigned long)sizeof({s}));')
        lines += [f'    printf("F {s} {f} %lu %lu\\n", (unsigned long)offsetof({s}, {f}), (unsigned long)sizeof((({s}*)0)->{f}));' for _, f in fields]
    lines += [f'    printf("C {c} %lld\\n", (long long)({c}));' for c in consts] + ["    return 0;", "}"]
    src = tmp_path_factory.mktemp("abi") / "abi_probe.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", D.INCLUDE, str(src), "-o", str(src.with_suffix(""))], check=True)
    out = {}
    for *key, last in (ln.split() for ln in subprocess.run([str(src.with_suffix(""))], capture_output=True, text=True, check=True).stdout.splitlines()):
        out[" ".join(key[:3])] = (int(key[3]), int(last)) if key[0] == "F" else int(last)
    return structs, consts, out


def test_structure_layouts_are_the_compilers(probe):
    structs, _, out = probe
    for s, fields in structs.items():
        st = getattr(_ffi, D.STRUCTS[s])
        assert len(st._fields_) == len(fields) and C.sizeof(st) == out[f"S {s}"], f"{s}: {len(fields)} fields, {out[f'S {s}']} bytes in C"
        for i, ((c_type, name), (py_name, ct)) in enumerate(zip(fields, st._fields_)):
            assert py_name == name, f"{s}: field {i} is `{name}` in the header, `{py_name}` in the Structure"
            got = (getattr(st, name).offset, getattr(st, name).size)
            assert got == out[f"F {s} {name}"], f"{s}.{name}: (offset, size) {got} in ctypes, {out[f'F {s} {name}']} in C"
            assert D.matches(c_type, ct, _ffi), f"{s}.{name}: `{c_type}` in the header, {ct.__name__} in the Structure"
    assert [out[f"S {s}"] for s in D.STRUCTS] == [40, 32, 72, 168]


def test_every_constant_has_the_headers_value(probe):
    _, consts, out = probe
    tw = twins()
    assert not set(tw) & set(UNUSED) and set(tw) | set(UNUSED) == set(consts), (set(tw) | set(UNUSED)) ^ set(consts)
    for name, value in tw.items():
        assert out[f"C {name}"] == value, f"{name}: {out[f'C {name}']} in the header, {value} in _ffi"
