#!/usr/bin/env python
"""Writes tests/golden/own_row_loads/<group>.npz from the library that is loaded (GMG_LIB_PATH or the tree's): the iterates and residues of
tests/own_row_loads_cases.py.  The committed fixtures were written with the build of the commit BEFORE the SELL row-dot kernels moved a row's
own operand loads in front of its dot product; tests/test_gpu_own_row_loads.py replays them bit for bit.

    python scripts/record_own_row_loads.py [--out DIR] [group ...]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gravo_mg_amd import cabi  # noqa: E402
from tests import own_row_loads_cases as oc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, oc.GOLDEN_DIR))
    ap.add_argument("groups", nargs="*", default=list(oc.GROUPS))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    print(f"library: {cabi.LIB_PATH}", flush=True)
    for group in args.groups:
        t0 = time.time()
        store = {}
        for name, d, stop_type, kw in oc.cases(group):
            P, rhs = oc.problem(group, d)
            eng = oc.engine(cabi, P, kw)
            try:
                fields = oc.run(eng, rhs, stop_type)
                info = [eng.level_info(k)["n"] if "n" in eng.level_info(k) else None for k in range(eng.num_levels)]
            finally:
                eng.close()
            assert np.array_equal(oc.bits(fields["first_x"]), oc.bits(fields["first_dev"])), (group, name)
            store.update(oc.pack(name, fields))
            print(f"  {group}/{name}: levels {info} solve iterations {int(fields['solve_it'][0])} residues {fields['cycles_hist']}", flush=True)
        path = os.path.join(args.out, f"{group}.npz")
        np.savez(path, **store)
        print(f"{group}: {len(store)} arrays, {os.path.getsize(path)} bytes, {time.time() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    main()
