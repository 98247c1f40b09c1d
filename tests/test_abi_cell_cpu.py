"""The per-cell ABI: include/acgan_cell.h against _lib.CELL_SIGNATURES position by position (the rules of tests/abi.py, through a
parser of this header), the three versions in the headers, the binding and the library, the other two headers left where they
were, and a call that is refused before a launch.  Neither the number of declarations nor the list of names is pinned: the
next per-cell score adds its entry point here."""
import os
import re

import abi
from dtgan_amd import _lib

HEADER = os.path.join(abi.ROOT, "include", "acgan_cell.h")
VERIF = os.path.join(abi.ROOT, "include", "acgan_verif.h")


def _source():
    """the header without comments and preprocessor lines (abi.source's rules)"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return re.sub(r"(?m)^\s*#.*$", " ", re.sub(r"//[^\n]*", " ", text))


def _declarations():
    """entry point -> (return kind, [argument kinds]), as abi.declarations reads them"""
    out = {}
    for ret, name, args in re.findall(r"([\w\s\*]+?)\b(acg_\w+)\s*\(([^()]*)\)\s*;", _source().replace('extern "C" {', " ")):
        args = [a.strip() for a in args.split(",")]
        out[name] = (abi._kind(ret), [] if args == ["void"] else [abi._kind(re.fullmatch(r"(.*?)\w+", a, flags=re.S).group(1)) for a in args])
    return out


def _version(path, name):
    return int(re.search(r"(?m)^#define\s+%s\s+(\d+)\s*$" % name, open(path).read()).group(1))


def test_binding_has_the_header_kinds_in_every_position():
    decl = _declarations()
    assert list(decl) == list(_lib.CELL_SIGNATURES)                # the same names in the same order, however many
    for name, (ret, args) in decl.items():
        res, argtypes = _lib.CELL_SIGNATURES[name]
        assert abi.kind_of(res) == ret, name
        assert [abi.kind_of(a) for a in argtypes] == args, name
    assert decl["acg_cell_version"] == ("int", [])
    assert decl["acg_cell_stats"] == ("int", ["ptr", "ptr"] + ["int"] * 5 + ["long long", "int", "long long"] * 2
                                      + ["ptr", "int", "ptr", "int"] + ["ptr"] * 5)


def test_three_versions_agree_and_the_other_headers_did_not_move():
    lib = _lib.load()
    assert _version(HEADER, "ACG_CELL_VERSION") == _lib.CELL_ABI_VERSION == lib.acg_cell_version() == 1
    assert _version(VERIF, "ACG_VERIF_VERSION") == _lib.VERIF_ABI_VERSION == lib.acg_verif_version()
    assert abi.header_version() == _lib.ABI_VERSION == lib.acg_version()
    names = set(_lib.CELL_SIGNATURES)
    assert not names & set(_lib.SIGNATURES) and not names & set(_lib.VERIF_SIGNATURES) and not names & set(abi.declarations())
    assert "acgan_cell.h" not in open(abi.HEADER).read() and "acgan_cell.h" not in open(VERIF).read()
    text = open(HEADER).read()
    assert "acgan_hip.h" in text and "#include \"acgan_hip.h\"" not in text and "#include \"acgan_verif.h\"" not in text   # it stands alone
    assert [t[1:4] for t in _lib._tables()] == [("acg_version", _lib.ABI_VERSION, None), ("acg_verif_version", 1, "include/acgan_verif.h"),
                                                ("acg_cell_version", 1, "include/acgan_cell.h")]


def test_call_and_query_reach_the_new_names():
    assert _lib.query("acg_cell_version") == 1
    try:
        _lib.call("acg_cell_stats", None, None, 0, 1, 1, 8, 8, 64, 1, 64, 64, 1, 64, None, 0, None, 0, None, None, None, None, None)
    except _lib.AcgError as e:
        assert "acg_cell_stats failed (-1): acg_cell_stats: need rows >= 1" in str(e)
    else:
        raise AssertionError("rows = 0 passed")
    for args, word in (((None, None, 2, 1, 1, 8, 8, 0, 1, 64, 64, 1, 64), "strides"), ((None, None, 3, 2, 1, 8, 8, 64, 1, 64, 64, 1, 64), "x_per_y"),
                       ((None, None, 2, 1, 1, 8, 8, 64, 1, 64, 64, 1, 64), "null")):
        try:
            _lib.call("acg_cell_stats", *(args + (None, 0, None, 0, None, None, None, None, None)))
        except _lib.AcgError as e:
            assert "acg_cell_stats: " in str(e) and word in str(e), (word, str(e))
        else:
            raise AssertionError(word)


def test_a_library_without_the_symbols_asks_for_a_rebuild(monkeypatch):
    """the loop over the tables keeps the messages of the two blocks it replaced"""
    import pytest
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.CELL_SIGNATURES, "acg_cell_missing", (_lib.c_int, []))
    with pytest.raises(_lib.AcgError, match=r"does not export acg_cell_missing \(include/acgan_cell.h\) — rebuild it \(make -C "):
        _lib.load()
    monkeypatch.delitem(_lib.CELL_SIGNATURES, "acg_cell_missing")
    monkeypatch.setattr(_lib, "VERIF_ABI_VERSION", 7)
    with pytest.raises(_lib.AcgError, match=r"reports verification ABI version 1, this binding expects 7 — rebuild it \(make -C "):
        _lib.load()
    monkeypatch.setattr(_lib, "VERIF_ABI_VERSION", 1)
    monkeypatch.setattr(_lib, "ABI_VERSION", 5)
    with pytest.raises(_lib.AcgError, match=r"reports ABI version 118, this binding expects 5 — rebuild it \(make -C "):
        _lib.load()
    monkeypatch.setattr(_lib, "ABI_VERSION", 118)
    assert _lib.load().acg_cell_version() == 1
