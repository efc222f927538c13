"""The SELL row-dot kernels (gs_color*, spmv_full*, transfer*, residual_norm_slices*) request a row's own operands -- diag, b, x_i / y_i, weight --
before the row's dot product instead of after it.  That moves loads and nothing else: every iterate and residue of
tests/own_row_loads_cases.py must have the bits that the build before the change produced (tests/golden/own_row_loads/*.npz, written by
scripts/record_own_row_loads.py from that build)."""
import os

import numpy as np
import pytest

from tests import own_row_loads_cases as oc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("group", oc.GROUPS)
def test_same_bits_as_before_the_loads_moved(cabi, group):
    golden = np.load(os.path.join(ROOT, oc.GOLDEN_DIR, f"{group}.npz"))
    compared, seen = 0, set()
    for name, d, stop_type, kw in oc.cases(group):
        P, rhs = oc.problem(group, d)
        eng = oc.engine(cabi, P, kw)
        try:
            fields = oc.run(eng, rhs, stop_type)
        finally:
            eng.close()
        # a solve that stops at its first check leaves x the iterate that was checked: the one it returns
        assert np.array_equal(oc.bits(fields["first_x"]), oc.bits(fields["first_dev"])), name
        compared += oc.check(name, fields, golden)
        seen.update(k for k in golden.files if k.startswith(name + "/"))
    assert seen == set(golden.files)          # every stored array was compared
    print(f"\n[own_row_loads] {group}: {len(oc.cases(group))} cases, {compared} values bit for bit")
