"""CPU: the oracle at every shape of the w4a16 route table (tests/w4a16_route_table.py) against an independent
high-precision value, through the same bounds the GPU test applies to the kernels (tests.util.assert_gemm_close
at its defaults), so that a GPU failure at one of these shapes (non-power-of-two groups, n = 8, k = 32, ...)
cannot be blamed on the reference.

Independent: the dequantised weights come from another unpacking path than the oracle's GEMM uses (AWQ:
R.awq_dequantize on the original AWQ layout instead of the exllama layout; GPTQ: the raw integers the inputs were
packed from, the act-order permutation applied to them directly), multiplied in float64 and rounded once to
the output type.
"""
import re

import pytest
import torch

from tests.util import ROOT, assert_gemm_close
from tests.w4a16_route_table import DTYPES, ROUTE_BITS, ROWS, case, row_id

from oracle import ref_ops as R  # noqa: E402


def test_route_bits_match_the_header_and_the_op_surface():
    txt = (ROOT / "include" / "mi355x_hotpath.h").read_text()
    header = {name: int(val) for name, val in re.findall(r"\bMI355X_W4_ROUTE_([A-Z0-9_]+)\s*=\s*(\d+)", txt)}
    assert header == ROUTE_BITS
    from vllm_metax_amd import _custom_ops as ops
    assert {name: getattr(ops, "W4_ROUTE_" + name) for name in ROUTE_BITS} == ROUTE_BITS


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("index", range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_oracle_against_float64_of_independently_dequantised_weights(index, dtype):
    quant, _, m, k, n, group, _, _ = ROWS[index]
    c = case(index, dtype)
    if quant.startswith("awq"):
        wd = R.awq_dequantize(c.qw, c.sc, c.qz)
        xx = c.x
    else:
        w, xx = c.w, c.x
        if c.perm is not None:
            w, xx = w[c.perm.long().numpy()], c.x[:, c.perm.long()]
        wd = R.w4_dequant(w, c.z.astype("int32") + 1, c.sc, group)
    assert wd.shape == (k, n) and wd.dtype == dtype
    indep = (xx.double() @ wd.double()).to(dtype)
    assert c.ref.shape == (m, n)
    assert_gemm_close(c.ref, indep, f"oracle {row_id(ROWS[index])}")
