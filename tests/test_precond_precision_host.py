"""gmg_config::precond_precision, the part that needs no device: the configuration mirror (the field stands directly in front of nullspace), its
default, the refusals gmg_create makes before it looks for a device -- with the codes and a message that names the field --, the combinations
that are allowed, and the drop-in's option.  The pattern is that of tests/test_pcg_host.py."""
import ctypes as C
import os
import sys

import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "gravo_mg_amd", "dropin")


def test_config_mirror_has_the_field_in_front_of_nullspace(cabi):
    names = [f[0] for f in cabi.GmgConfig._fields_]
    assert names[-8:] == ["precond_precision", "nullspace", "fold_head", "reorder_pointwise", "zero_guess_step", "pcg", "device_coloring", "accelerate"]
    assert cabi.GmgConfig._fields_[-8] == ("precond_precision", C.c_int)
    assert C.sizeof(cabi.GmgConfig) == cabi.lib().gmg_config_size()
    cfg = cabi.GmgConfig()
    cfg.precond_precision = 7
    cfg.nullspace = 5
    assert cabi.lib().gmg_config_default(C.byref(cfg)) == 0 and cfg.precond_precision == 0 and cfg.nullspace == 0 and cfg.pcg == 0


def test_no_entry_point_was_added(cabi):
    assert len(cabi.SIGNATURES) == 75


def _refused(cabi, **kw):
    with pytest.raises(cabi.GmgError) as ei:
        cabi.Engine(**kw)
    return ei.value


def test_create_refuses_without_a_device(cabi):
    """Every refusal comes before the device is looked for: the same codes on a machine without a GPU."""
    cheb = cabi.SMOOTHER_CHEBYSHEV
    for bad in (-1, 2, 100):
        e = _refused(cabi, pcg=1, smoother=cheb, precond_precision=bad)
        assert e.code == cabi.GMG_ERR_INVALID and "precond_precision" in str(e), (bad, str(e))
        e = _refused(cabi, precond_precision=bad)
        assert e.code == cabi.GMG_ERR_INVALID and "precond_precision" in str(e), (bad, str(e))
    # the field is the precision of the CG loop's cycle: without that loop there is nothing it could mean
    for kw in (dict(precond_precision=1), dict(precond_precision=1, smoother=cheb), dict(precond_precision=1, inner_precision=1),
               dict(precond_precision=1, accelerate=2), dict(precond_precision=1, pcg=0, smoother=cabi.SMOOTHER_JACOBI)):
        e = _refused(cabi, **kw)
        assert e.code == cabi.GMG_ERR_UNSUPPORTED and "precond_precision" in str(e), (kw, str(e))
    # pcg's own rules hold with the field set: the existing refusals, which name pcg
    for kw in (dict(pcg=1, precond_precision=1), dict(pcg=1, precond_precision=1, smoother=cheb, inner_precision=1),
               dict(pcg=1, precond_precision=1, smoother=cheb, accelerate=1), dict(pcg=1, precond_precision=1, smoother=cheb, pre_iters=2, post_iters=1)):
        e = _refused(cabi, **kw)
        assert e.code == cabi.GMG_ERR_UNSUPPORTED and "pcg" in str(e), (kw, str(e))
    allowed = [dict(pcg=1, smoother=cheb, precond_precision=1), dict(pcg=1, smoother=cabi.SMOOTHER_JACOBI, precond_precision=1, pre_iters=1, post_iters=1),
               dict(pcg=1, smoother=cheb, precond_precision=1, pre_iters=3, post_iters=3, use_graph=True),
               dict(pcg=1, smoother=cheb, precond_precision=1, nullspace=1, zero_guess_step=1, reorder_pointwise=1),
               dict(pcg=1, smoother=cheb, precond_precision=0), dict(precond_precision=0), dict(precond_precision=0, inner_precision=1)]
    allowed += [dict(pcg=1, smoother=cheb, precond_precision=1, coarse_mode=m) for m in (0, 1, 2, 3)]
    for kw in allowed:
        try:
            cabi.Engine(**kw).close()
        except cabi.GmgError as e:
            assert cabi.device_count() == 0 and e.code == cabi.GMG_ERR_NO_DEVICE, (kw, str(e))
    # a refusal's message does not outlive the next gmg_create of the thread
    e = _refused(cabi, accelerate=9)
    assert e.code == cabi.GMG_ERR_INVALID and "precond_precision" not in str(e)


def test_dropin_accepts_the_option(cabi):
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
    solver.set_engine_option("pcg", 1)
    solver.set_engine_option("precond_precision", 1)
    with pytest.raises(Exception):
        solver.set_engine_option("precond_precision_more", 1)
    assert "precond_precision" in gravomg.MultigridSolver.set_engine_option.__doc__
