"""Shared pieces of the C-ABI return-code tests: the header's prototypes, the error codes and the table runner.

TEST INFRASTRUCTURE.  A return-code table is a base dict -- one accepted call of an entry point, its keys the
parameter names of include/simamba.h in the header's order -- and rows ``(change, want)``: what the row changes in
that call, and the code the library answers.  The call passes the dict's values positionally, and ctypes takes surplus
arguments silently and converts whatever it is given, so ``check_rows`` holds the keys to the header first: a table with
two keys swapped, one missing or one misspelt fails there, not by landing a value in the wrong slot.
"""
import functools
import os
import re

from conftest import ROOT
from si_mamba_amd import _lib

P = 1 << 20     # a 16-byte aligned, non-null address, never dereferenced: every call with it ends in validation
OFF = P + 4     # the same, 4 bytes off the alignment
# The numbers are an ABI promise: literal here, pinned to the header's SIMAMBA_E_* by tests/test_abi.py.
OK = 0
E_NULLPTR, E_SHAPE, E_DTYPE, E_DSTATE, E_WIDTH, E_WORKSPACE, E_GROUPS, E_ALIGN, E_VARIANT, E_BIAS = \
    -1, -2, -3, -4, -5, -6, -7, -8, -9, -10


def header_code():
    """include/simamba.h with its comments stripped."""
    with open(os.path.join(ROOT, "include", "simamba.h")) as fh:
        text = fh.read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


@functools.lru_cache(maxsize=None)
def declared_params():
    """name -> the parameter declarations of every simamba_* prototype in the header, comments stripped."""
    out = {}
    for name, params in re.findall(r"\b(simamba_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header_code()):
        assert name not in out, name
        params = [p.strip() for p in params.split(",")]
        out[name] = [] if params == ["void"] else params
    return out


def param_names(name):
    """The parameter names of the entry point ``name``, in the header's order."""
    return [re.search(r"(\w+)$", p).group(1) for p in declared_params()[name]]


def checked_call(name, base, change, lib=None):
    """-> the code ``name`` answers to ``base`` changed by ``change``.  Nothing is called unless ``base`` spells the
    header's parameter names in order and ``change`` changes only parameters that exist."""
    keys, names = list(base), param_names(name)
    if keys != names:
        i = next((i for i, (k, n) in enumerate(zip(keys, names)) if k != n), min(len(keys), len(names)))
        have = repr(keys[i]) if i < len(keys) else "nothing"
        want = repr(names[i]) if i < len(names) else "nothing"
        raise AssertionError(f"{name}: argument {i} of the table is {have}, include/simamba.h declares {want} "
                             f"({len(keys)} keys, {len(names)} parameters)")
    assert set(change) <= set(base), (name, change, sorted(set(change) - set(base)))
    return getattr(lib if lib is not None else _lib.load(), name)(*{**base, **change}.values())


def check_rows(name, base, rows, lib=None):
    """Every row ``(change, want)`` of a return-code table: ``name`` called with ``base`` changed by ``change`` answers
    ``want``."""
    for change, want in rows:
        got = checked_call(name, base, change, lib)
        assert got == want, (name, change, got)
