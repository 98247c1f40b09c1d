"""The ctypes binding against the header, completely and once: every entry point's return and argument kinds, every struct's
fields, the version.  A c_int where the header says `long long`, or a c_float where it says `double`, shifts every later
argument silently; _lib.ABI_VERSION only guards against a stale build, not against a binding written wrongly.  The per-feature
*_cpu.py tests pin what is particular to their entry points through abi.header_args.  Also the guard that keeps test modules
from being used as libraries."""
import glob
import os
import re

import pytest

import abi
from dtgan_amd import _lib

STRUCTS = {"acg_conv_desc": _lib.ConvDesc, "acg_pack_item": _lib.PackItem, "acg_norm_sums": _lib.NormSumsDesc,
           "acg_segments": _lib.Segments, "acg_latent_mlp_params": _lib.LatentMlpParams,
           "acg_latent_mlp_grads": _lib.LatentMlpGrads, "acg_adam_group": _lib.AdamGroup, "acg_ema_group": _lib.EmaGroup,
           "acg_window_plan": _lib.WindowPlan}


@pytest.mark.parametrize("name", sorted(abi.declarations()))
def test_binding_has_the_header_kinds_in_every_position(name):
    ret, args = abi.declarations()[name]
    assert name in _lib.SIGNATURES, "%s is declared in the header and not bound" % name
    res, argtypes = _lib.SIGNATURES[name]
    assert abi.kind_of(res) == ret, "%s returns %s in the header, %s in _lib.SIGNATURES" % (name, ret, abi.kind_of(res))
    bound = [abi.kind_of(a) for a in argtypes]
    assert len(bound) == len(args), "%s takes %d arguments in the header, %d in _lib.SIGNATURES" % (name, len(args), len(bound))
    wrong = ["argument %d: header %s, binding %s" % (i, h, b) for i, (h, b) in enumerate(zip(args, bound)) if h != b]
    assert not wrong, "%s: %s" % (name, "; ".join(wrong))


def test_header_and_binding_name_the_same_entry_points():
    assert set(abi.declarations()) == set(_lib.SIGNATURES), set(abi.declarations()) ^ set(_lib.SIGNATURES)
    assert len(abi.declarations()) == 128


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_structure_has_the_header_fields(name):
    assert abi.structure_fields(STRUCTS[name]) == abi.structs()[name]


def test_every_struct_of_the_header_is_checked():
    assert set(abi.structs()) == set(STRUCTS)
    assert abi.structs()["acg_latent_mlp_params"][:2] == [("w", "ptr", 4), ("b", "ptr", 4)]      # `const float *w[4], *b[4], ...;`
    assert abi.structs()["acg_segments"][1:3] == [("off", "int", 96), ("len", "int", 96)]        # ACG_MAX_SEGMENTS resolved


def test_version_is_one_number_in_the_header_the_binding_and_the_library():
    assert abi.header_version() == _lib.ABI_VERSION == _lib.load().acg_version() == 118


def test_no_test_file_imports_from_a_test_module():
    """helpers live in modules that are not collected (field_cases, model_cases, eval_cases, conv_cases, *_ref, *_util): a
    test module that serves as a library breaks the collection of its users when it is edited"""
    here = os.path.dirname(os.path.abspath(__file__))
    found = []
    for path in sorted(glob.glob(os.path.join(here, "*.py"))):
        for i, line in enumerate(open(path), 1):
            if re.match(r"\s*(from\s+test_\w*\s+import\b|import\s+(\w+\s*,\s*)*test_\w*)", line):
                found.append("%s:%d: %s" % (os.path.basename(path), i, line.strip()))
    assert not found, "\n".join(found)
