"""sqfa_airm_options::launch_policy on the host side: the ctypes mirror matches the header field for field, the new field is
last (a structure built from the four earlier fields means "default"), and the per-call policy reaches the structure."""
import os
import re

import pytest

from conftest import ROOT


def header_fields():
    text = open(os.path.join(ROOT, "include", "sqfa_hip.h")).read()
    body = re.search(r"typedef struct sqfa_airm_options \{(.*?)\} sqfa_airm_options;", text, re.S).group(1)
    return [re.sub(r"^\*", "", decl.split()[-1]) for decl in body.split(";") if decl.strip()]


def test_ctypes_structure_mirrors_the_header():
    from sqfa_amd import _lib
    names = [f[0] for f in _lib.AirmOptions._fields_]
    assert names == header_fields()
    assert names[-1] == "launch_policy"
    assert _lib.AirmOptions(0, 0, None, 0).launch_policy == 0   # four fields given: the default policy


def test_policy_reaches_the_options():
    from sqfa_amd import _native
    assert _native._options().launch_policy == 0
    with _native.policies(launch=-1):
        assert _native._options().launch_policy == -1
        with _native.policies(launch=1, class_factor=1):
            opts = _native._options()
            assert (opts.launch_policy, opts.class_factor_policy) == (1, 1)
    assert _native._options().launch_policy == 0
    with pytest.raises(TypeError):
        _native.policies(launches=0)


def test_header_names_the_policy_bits():
    text = open(os.path.join(ROOT, "include", "sqfa_hip.h")).read()
    assert re.search(r"#define SQFA_LAUNCH_FUSED_PROLOGUE\s+1\b", text) and re.search(r"#define SQFA_LAUNCH_FUSED_REDUCTION\s+2\b", text)
