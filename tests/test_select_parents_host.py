"""The host routine of the per-point parent selection (HierarchyBuilder::select_point, through gmg_debug_select_parents mode 0) against
the Python restatement (oracle/hierarchy_restatement.py::select_point) on the branch catalogue of tests/select_cases.py: every case
reaches the branch it was built for, same parents in the same order, same weights.  CPU only; tests/test_gpu_select_parents.py holds the
device kernel against both on the same cases."""
import numpy as np
import pytest

from tests import select_cases as sc


@pytest.mark.parametrize("name,builder,args", sc.CASES, ids=sc.CASE_IDS)
def test_host_routine_matches_restatement_on_the_branch_catalogue(cabi, name, builder, args):
    sc.check_host(cabi, builder(*args))


def test_host_keeps_the_signed_zero_of_the_unclamped_edge_parameter(cabi):
    """emit_edge's std::max(w2, 0.) keeps w2 = -0.0 (the point on its own cell position, all three components of the edge vector negative):
    the bit pattern the device stage has to reproduce."""
    job = sc.one_neighbour(0)
    _, _, _, w = job.run(cabi, 0)
    f = next(i for i in range(job.nf) if job.P[i].tolist() == [4, 4, 4])
    assert w[f].view(np.uint64)[:2].tolist() == [0x3FF0000000000000, 0x8000000000000000]


def test_device_modes_fail_loudly_without_a_gpu(cabi):
    if cabi.device_count() > 0:
        pytest.skip("a HIP device is present")
    job = sc.launch_edges(1)
    for mode in (1, 2):
        with pytest.raises(cabi.GmgError) as ei:
            job.run(cabi, mode)
        assert ei.value.code == cabi.GMG_ERR_NO_DEVICE


def test_bad_indices_are_rejected(cabi):
    job = sc.containing_triangle(0)
    job.nearest[3] = job.nc
    with pytest.raises(cabi.GmgError) as ei:
        job.run(cabi, 0)
    assert ei.value.code == cabi.GMG_ERR_INVALID
