"""CPU: the binding tables of the latent-input entries against their headers' prototypes, and the long-double restatement's dL/dX
against central differences of its own log marginal likelihood."""
import os
import re

import numpy as np
import pytest

import kern_ld as KL
import latent_ld as LL
from gpy_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"int": _lib._ci, "int64_t": _lib._i64, "double": _lib._cd}


@pytest.mark.parametrize("header,table", [("mi355gp_latent.h", "LATENT_ABI"), ("mi355gp_debug_latent.h", "DEBUG_LATENT_ABI")])
def test_the_binding_table_states_the_headers_prototypes(header, table):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    protos = re.findall(r"\bint\s+(mi355gp_\w+)\s*\(([^)]*)\)\s*;", text)
    abi = getattr(_lib, table)
    assert [name for name, _ in protos] == list(abi)
    for name, args in protos:
        kinds = []
        for a in (x.strip() for x in args.split(",")):
            if "*" in a:
                kinds.append("ptr")
            else:
                kinds.append(CTYPE[a.split()[-2]])
        got = [t if t in CTYPE.values() else "ptr" for t in abi[name]]
        assert got == kinds, name
    assert all(hasattr(_lib.Context, m) for m in ("latent_set_X", "latent_inference_sum")) and callable(_lib.dbg_latent_grad)


@pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")
def test_the_restatements_dX_agrees_with_central_differences_of_its_own_lml():
    rng = np.random.RandomState(5)
    X, Y = rng.rand(9, 2) * 3.0, rng.randn(9, 4)
    specs = [LL.spec("matern52", 1, [1.1, 0.8, 1.3], [0, 1]), LL.spec("bias", 0, [0.2], [0, 1])]
    ref = LL.evaluate(specs, X, Y, 0.3)
    h = KL.LD(1e-7)
    for i, q in ((0, 0), (4, 1), (8, 0)):
        Xp, Xm = np.array(X, dtype=KL.LD), np.array(X, dtype=KL.LD)
        Xp[i, q] += h
        Xm[i, q] -= h
        num = (LL.evaluate(specs, Xp, Y, 0.3)["lml"] - LL.evaluate(specs, Xm, Y, 0.3)["lml"]) / (2 * h)
        assert abs(num - ref["dX"][i, q]) <= 1e-9 * np.max(np.abs(ref["dX"]))      # the difference's own h^2 term, ~1e-14 relative
