"""The device kernel of the per-point parent selection (gmgh::select_parents, csrc/hierarchy_kernels.hip.hpp) branch by branch at
small sizes, through gmg_debug_select_parents -- the builder's own upload / launch / download -- on the hand-built catalogue of
tests/select_cases.py.  Every case asserts
  (a) device records == host records bit for bit (cnt, kind, col[:cnt], w[:cnt] as uint64: a signed zero counts);
  (b) the builder's combination (device records, handed-back points redone on the host) == host records on every point;
  (c) host and device agree with the Python restatement (same parents in the same order, weights to rtol 1e-9 / atol 1e-12);
  (d) every point reached the branch it was built for.
The last test crosses the 16 MB bounce pieces of the transfer code (HierarchyXfer::up / down, engine.hip)."""
import numpy as np
import pytest

from tests import select_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,builder,args", sc.CASES, ids=sc.CASE_IDS)
def test_device_selection_matches_host_and_restatement_on_the_branch_catalogue(cabi, name, builder, args):
    job = builder(*args)
    host = sc.check_host(cabi, job)              # (c) for the host, (d)
    sc.check_device(cabi, job, host)             # (a), (b), (c) for the device


@pytest.mark.parametrize("weighting", [0, 2])
def test_transfers_across_a_bounce_piece(cabi, weighting):
    """700 001 points over a hand-built 40 x 40 triangulated coarse grid.  The transfer code moves every array in 16 MB pieces through
    two pinned buffers with event reuse: at this size the positions P going up and the weights w coming down (24 bytes per point each,
    16 MB = 699 051 points) take a second piece.  col (12 bytes per point) would need 1.4 M points, cnt and kind (1 byte) 16.8 M: they
    stay in one piece here.  (a) and (b) over all points, (c) over a fixed random sample of 2 000."""
    nf = 700_001
    job = sc.coarse_grid_job(nf, weighting)
    assert job.P.nbytes > 16 * 2**20 > 12 * nf
    sample = np.sort(np.random.default_rng(99).choice(nf, 2000, replace=False))
    host = sc.check_host(cabi, job, sample)
    kinds = np.bincount(host[1], minlength=5)
    print(f"row kinds of the {nf} points (triangle / edge / closest three / single / nested): {kinds.tolist()}")
    assert kinds[sc.TRIANGLE] > 0 and kinds[sc.EDGE] > 0 and kinds[sc.CLOSEST] > 0
    sc.check_device(cabi, job, host, sample)
