"""How many instantiations of each kernel template the built library holds, against the counts recorded from the library before the launchers
chose their template forms through the constant dispatcher of csrc/common.h (tests/golden/kernel_families.json).

A launcher built on with_flags / with_one_of instantiates every combination of its flags that its `if constexpr (..._form_built(...))` guard
lets through.  A guard that lets through too much fails nothing else: the extra kernels are never launched, they only lengthen the build and
the code object.  A guard that lets through too little does not link a form an entry can reach.  Either shows here as a count that moved.

Read from the library's own metadata (tools/kernel_resources.py); a family is the kernel's name in front of its template arguments, taken
from the mangled name (the demangler leaves the bf16 kernels' names alone)."""
import collections
import json
import os
import re

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_families.json")


def family(mangled):
    """_ZN12_GLOBAL__N_118series_gemm_kernelILi1ELb1E...EEvT_ -> series_gemm_kernel: the last length-prefixed name of the (nested) name"""
    s = mangled[3:] if mangled.startswith("_ZN") else mangled[2:]
    name = None
    while s[:1].isdigit():
        n = re.match(r"\d+", s)
        end = n.end() + int(n.group())
        name, s = s[n.end():end], s[end:]
    return name


def families(resources):
    return dict(collections.Counter(family(k) for k in resources))


def test_family_of_a_mangled_name():
    assert family("_ZN12_GLOBAL__N_118series_gemm_kernelILi1ELb1ELb0ELb0ELb0ELb0EEEvNS_16SeriesGemmParamsE") == "series_gemm_kernel"
    assert family("_ZN12_GLOBAL__N_123series_gemm_bf16_kernelILi4ELb1ELb0EDF16bLb1ELb0EEEvNS_20SeriesGemmBf16ParamsE") == "series_gemm_bf16_kernel"
    assert family("_ZN12_GLOBAL__N_119wgrad_reduce_kernelENS_11WgradParamsE") == "wgrad_reduce_kernel"
    assert family("_Z7plain_kPf") == "plain_k"


def test_instantiations_per_kernel_family():
    from tgcn_amd import _lib
    from tools import kernel_resources as kr
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")):
        pytest.skip("needs the built library and llvm-readelf")
    with open(GOLDEN) as f:
        want = json.load(f)
    have = families(kr.kernel_resources(_lib.LIB_PATH))
    moved = {k: (have.get(k, 0), want["families"].get(k, 0)) for k in set(have) | set(want["families"]) if have.get(k, 0) != want["families"].get(k, 0)}
    assert not moved, "family: (built, recorded) %s" % sorted(moved.items())
    assert sum(have.values()) == want["kernels"]
