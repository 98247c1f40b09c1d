"""The verification-only ABI: include/acgan_verif.h against _lib.VERIF_SIGNATURES position by position (the rules of
tests/abi.py, through a parser of this header), its version in the header, the binding and the library, the training header
left where it was, and the workspace query's refusals."""
import os
import re

import abi
from dtgan_amd import _lib

HEADER = os.path.join(abi.ROOT, "include", "acgan_verif.h")


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


def _version():
    return int(re.search(r"(?m)^#define\s+ACG_VERIF_VERSION\s+(\d+)\s*$", open(HEADER).read()).group(1))


def test_binding_has_the_header_kinds_in_every_position():
    decl = _declarations()
    assert list(decl) == ["acg_verif_version", "acg_reliability_workspace_bytes", "acg_reliability"]
    assert set(decl) == set(_lib.VERIF_SIGNATURES)
    for name, (ret, args) in decl.items():
        res, argtypes = _lib.VERIF_SIGNATURES[name]
        assert abi.kind_of(res) == ret, name
        assert [abi.kind_of(a) for a in argtypes] == args, name
    assert decl["acg_reliability_workspace_bytes"] == ("size_t", ["int"] * 7)
    assert decl["acg_reliability"][1] == (["ptr", "ptr"] + ["int"] * 5 + ["long long", "int", "long long"] * 2
                                          + ["ptr", "int", "ptr", "int", "ptr", "ptr", "size_t", "ptr"])


def test_versions_agree_and_the_training_abi_did_not_move():
    lib = _lib.load()
    assert _version() == _lib.VERIF_ABI_VERSION == lib.acg_verif_version() == 1
    assert len(abi.declarations()) == 128 and not set(abi.declarations()) & set(_lib.VERIF_SIGNATURES)
    assert not set(_lib.SIGNATURES) & set(_lib.VERIF_SIGNATURES) and len(_lib.SIGNATURES) == 128
    assert abi.header_version() == _lib.ABI_VERSION == lib.acg_version()
    assert "acgan_verif.h" not in open(abi.HEADER).read()          # the training header does not pull it in
    text = open(HEADER).read()
    assert "acgan_hip.h" in text and "#include \"acgan_hip.h\"" not in text   # it names it, and stands alone


def test_call_and_query_reach_the_new_names():
    assert _lib.query("acg_verif_version") == 1
    assert _lib.query("acg_reliability_workspace_bytes", 1, 1, 1, 1, 1, 1, 1) == 64      # two planes of a word and two prefixes, each part rounded to 16 bytes
    try:
        _lib.call("acg_reliability", None, None, 0, 1, 1, 8, 8, 64, 1, 64, 64, 1, 64, None, 1, None, 1, None, None, 0, None)
    except _lib.AcgError as e:
        assert "acg_reliability failed (-1): acg_reliability: need rows >= 1" in str(e)
    else:
        raise AssertionError("rows = 0 passed")


def test_workspace_query():
    """acg_fss's planes of x and of y, whatever the windows; 0 for every size the call refuses"""
    q = _lib.load().acg_reliability_workspace_bytes
    up = lambda n: (n + 15) // 16 * 16
    for H, W in ((1, 1), (5, 7), (64, 64), (65, 130), (321, 321), (1024, 1024)):
        WW = (W + 63) // 64
        planes = lambda n: up(n * H * WW * 8) + up(n * H * (WW + 1) * 2)
        assert q(4, 2, 3, H, W, 3, 6) == planes(36) + planes(18) == q(4, 2, 3, H, W, 3, 1)
        assert q(64, 64, 1, H, W, 1, 8) == planes(64) + planes(1)
        assert q(4, 1, 1, H, W, 8, 1) == 2 * planes(32)
    for bad in ((0, 1, 1, 8, 8, 1, 1), (2, 1, 0, 8, 8, 1, 1), (2, 0, 1, 8, 8, 1, 1), (130, 65, 1, 8, 8, 1, 1), (6, 4, 1, 8, 8, 1, 1),
                (2, 1, 1, 0, 8, 1, 1), (2, 1, 1, 8, 0, 1, 1), (2, 1, 1, 1025, 8, 1, 1), (2, 1, 1, 8, 1025, 1, 1), (2, 1, 1, 8, 8, 0, 1),
                (2, 1, 1, 8, 8, 9, 1), (2, 1, 1, 8, 8, 1, 0), (2, 1, 1, 8, 8, 1, 9), (1 << 30, 1, 4, 8, 8, 1, 1), (-1, 1, 1, 8, 8, 1, 1)):
        assert q(*bad) == 0, bad
