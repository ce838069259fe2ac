"""No GPU: the binding table of include/mi355gp_eigh.h, the export of the eigensolver under GPy's names and what
`gpy_amd.linalg.eigh` refuses before any device work."""
import os
import re

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib, linalg

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_binding_table_is_the_header():
    text = open(os.path.join(HERE, "..", "include", "mi355gp_eigh.h")).read()
    protos = re.findall(r"\bint\s+(mi355gp_\w+)\s*\(([^;]*?)\)\s*;", text)
    assert [p[0] for p in protos] == list(_lib.EIGH_ABI) == ["mi355gp_eigh"]
    params = [p.strip() for p in protos[0][1].split(",")]
    assert params == ["int device", "const double* A", "int64_t n", "double* w", "double* V", "int* sweeps", "double* ms"]
    assert len(_lib.EIGH_ABI["mi355gp_eigh"]) == len(params)
    for name, value in (("B", _lib.EIGH_B), ("MAX_SWEEPS", _lib.EIGH_MAX_SWEEPS), ("MAX_N", _lib.EIGH_MAX_N)):
        assert int(re.search(r"#define MI355GP_EIGH_%s (\d+)" % name, text).group(1)) == value


def test_exported_under_gpys_names():
    assert gpy_amd.util.linalg.eigh is linalg.eigh is gpy_amd.linalg.eigh


@pytest.mark.parametrize("A, what", [
    (np.zeros((3, 4)), "square"),
    (np.zeros(5), "square"),
    (np.array([[1.0, 0.5], [0.25, 1.0]]), "not symmetric"),
    (np.array([[1.0, np.nan], [np.nan, 1.0]]), "not finite"),
    (np.broadcast_to(0.0, (_lib.EIGH_MAX_N + 1,) * 2), "limit of %d" % _lib.EIGH_MAX_N),
])
def test_refused_by_name_before_any_device_work(monkeypatch, A, what):
    monkeypatch.setattr(_lib, "eigh", lambda *a, **k: pytest.fail("the device was reached"))
    with pytest.raises(ValueError, match=what):
        linalg.eigh(A)
