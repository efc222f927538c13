"""gmg_config::reorder_pointwise and gmg_config::zero_guess_step, the part that needs no device: the configuration mirror, the range checks
gmg_create makes before it looks for a device (gmg_last_error(NULL) names the field), the acceptance with every smoother, the drop-in's options."""
import ctypes as C
import os
import sys

import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "gravo_mg_amd", "dropin")
FIELDS = ("reorder_pointwise", "zero_guess_step")


def test_config_mirror_has_the_fields_behind_fold_head(cabi):
    """Behind fold_head, in front of pcg: the tail that tests/test_pcg_host.py, test_jp_coloring_host.py and test_accelerate_host.py pin stays."""
    names = [f[0] for f in cabi.GmgConfig._fields_]
    assert names[-5:] == ["reorder_pointwise", "zero_guess_step", "pcg", "device_coloring", "accelerate"]
    assert names[-6] == "fold_head"
    assert cabi.GmgConfig._fields_[-5] == ("reorder_pointwise", C.c_int) and cabi.GmgConfig._fields_[-4] == ("zero_guess_step", C.c_int)
    assert C.sizeof(cabi.GmgConfig) == cabi.lib().gmg_config_size()
    cfg = cabi.GmgConfig()
    cfg.reorder_pointwise, cfg.zero_guess_step = 7, 7
    assert cabi.lib().gmg_config_default(C.byref(cfg)) == 0
    assert cfg.reorder_pointwise == 0 and cfg.zero_guess_step == 0 and cfg.pcg == 0 and cfg.fold_head == 1


def _refused(cabi, **kw):
    with pytest.raises(cabi.GmgError) as ei:
        cabi.Engine(**kw)
    return ei.value


@pytest.mark.parametrize("field", FIELDS)
def test_values_other_than_0_and_1_are_refused_without_a_device(cabi, field):
    for smoother in (cabi.SMOOTHER_MULTICOLOR_GS, cabi.SMOOTHER_JACOBI, cabi.SMOOTHER_CHEBYSHEV):
        for bad in (2, -1):
            e = _refused(cabi, smoother=smoother, **{field: bad})
            assert e.code == cabi.GMG_ERR_INVALID and field in str(e), (smoother, bad, str(e))
    # the message names the field that was wrong, not its neighbour, and does not outlive the next gmg_create of the thread
    other = FIELDS[1 - FIELDS.index(field)]
    assert other not in str(_refused(cabi, **{field: 2, other: 1}))
    e = _refused(cabi, accelerate=9)
    assert e.code == cabi.GMG_ERR_INVALID and field not in str(e)


def test_every_smoother_accepts_the_fields(cabi):
    """Without a device that shows as GMG_ERR_NO_DEVICE only (with the multicolour smoother the fields are accepted and have no effect)."""
    for smoother in (cabi.SMOOTHER_MULTICOLOR_GS, cabi.SMOOTHER_JACOBI, cabi.SMOOTHER_CHEBYSHEV):
        for rp in (0, 1):
            for zg in (0, 1):
                for more in (dict(), dict(pre_iters=0, post_iters=2), dict(inner_precision=1), dict(accelerate=3), dict(use_graph=True)):
                    kw = dict(smoother=smoother, reorder_pointwise=rp, zero_guess_step=zg, **more)
                    try:
                        cabi.Engine(**kw).close()
                    except cabi.GmgError as e:
                        assert cabi.device_count() == 0 and e.code == cabi.GMG_ERR_NO_DEVICE, (kw, str(e))
    for smoother in (cabi.SMOOTHER_JACOBI, cabi.SMOOTHER_CHEBYSHEV):
        kw = dict(smoother=smoother, pcg=1, reorder_pointwise=1, zero_guess_step=1)
        try:
            cabi.Engine(**kw).close()
        except cabi.GmgError as e:
            assert cabi.device_count() == 0 and e.code == cabi.GMG_ERR_NO_DEVICE, (kw, str(e))
    # the refusals of pcg stand with the fields set
    e = _refused(cabi, pcg=1, reorder_pointwise=1, zero_guess_step=1)
    assert e.code == cabi.GMG_ERR_UNSUPPORTED and "pcg" in str(e)


def test_dropin_accepts_the_options(cabi):
    import glob
    if not glob.glob(os.path.join(DROPIN, "gravomg_bindings*.so")):
        import __graft_entry__
        __graft_entry__.build()
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import gravomg
    from gravo_mg_amd import meshgen
    V, F = meshgen.torus_mesh(24, 20)
    S, mass = meshgen.cotan_laplacian(V, F)
    solver = gravomg.MultigridSolver(V, gravomg.neighbors_from_stiffness(S), sp.diags(mass).tocsr(), lower_bound=40)
    for field in FIELDS:
        solver.set_engine_option(field, 1)
        with pytest.raises(Exception):
            solver.set_engine_option(field + "_more", 1)
        assert field in gravomg.MultigridSolver.set_engine_option.__doc__
