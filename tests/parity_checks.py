"""Checks shared by the GPU parity tests (tests/test_gpu_parity.py on the hierarchy builder's meshes, tests/test_gpu_boundary_shapes.py on
synthetic problems of exact shapes, tests/test_gpu_sweep_counts.py at other sweep counts): a device smoother against its matrix form built
from the oracle's arithmetic, the oracle on the device's colour ordering, which launch paths the timing keys say ran."""
import numpy as np
import scipy.sparse as sp

from tests import problems


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


def check_block_sweeps(P, eng, oracle, ds=(1, 3)):
    """Blocked levels: one sweep == x + T^-1 (b - A x) with T = D + strict-lower(A restricted to the block diagonal) in device order, <= 1e-12
    relative; the in-block colouring is proper and rows are colour-sorted inside a block.  Returns the number of blocked levels checked."""
    import scipy.sparse.linalg as spla
    rng = np.random.default_rng(7)
    checked = 0
    for k in range(len(P.U)):
        blocks = eng.level_blocks(k)
        if blocks is None:
            assert k == 0
            continue
        checked += 1
        blk_begin, row_color = blocks
        A = eng.level_operator(k)
        new2old, _ = eng.level_ordering(k)
        assert np.all(np.diff(blk_begin) % 64 == 0) and np.all(np.diff(blk_begin) <= 1024) and blk_begin[-1] == len(new2old)
        real = new2old >= 0
        blk_of_dev = np.repeat(np.arange(len(blk_begin) - 1), np.diff(blk_begin))
        order = new2old[real]; blk = blk_of_dev[real]; col = row_color[real]
        Ap = A.tocsr()[order][:, order].tocoo()
        same = blk[Ap.row] == blk[Ap.col]
        off = Ap.row != Ap.col
        # proper colouring inside every block, rows colour-sorted inside a block
        assert np.all(col[Ap.row[same & off]] != col[Ap.col[same & off]])
        assert np.all((np.diff(col) >= 0) | (np.diff(blk) != 0))
        keep = same & (Ap.col <= Ap.row)
        T = sp.csr_matrix((Ap.data[keep], (Ap.row[keep], Ap.col[keep])), shape=Ap.shape)
        for d in ds:
            b = rng.standard_normal((A.shape[0], d)); x = rng.standard_normal((A.shape[0], d))
            want = x.copy()
            for iters in (1, 2, 3, 4, 5):          # (both parities of the ping-pong between x and tmp, with and without a copy back)
                r = oracle.residual(A, b, want)
                step = np.empty_like(want)
                step[order] = spla.spsolve_triangular(T, r[order], lower=True)
                want = want + step
                got = eng.smooth(k, b, x, iters)
                assert rel(got, want) <= 1e-12
    assert checked == len(P.U) - (eng.level_blocks(0) is None)       # (level 0 too where the engine blocked it: block_from_level = 0, or gmg_config::block_fine on a kNN operator)
    return checked


def check_multicolor_gs(P, eng, oracle, ds=(1, 3)):
    """Exact engine (block_rows = 0, gs_omega = 1): the colouring of every level is proper, and its sweeps are the reference's lexicographic
    Gauss-Seidel on the colour-permuted system P A P^T, <= 1e-12 relative against the oracle run on P A P^T."""
    rng = np.random.default_rng(2)
    for k in range(len(P.U)):
        A = eng.level_operator(k)
        new2old, color_begin = eng.level_ordering(k)
        Ap, order = problems.permuted_system(A, new2old)
        # colouring is proper: no edge inside a colour class
        colour_of = np.empty(A.shape[0], int)
        for c in range(len(color_begin) - 1):
            rows = new2old[color_begin[c]:color_begin[c + 1]]
            colour_of[rows[rows >= 0]] = c
        coo = sp.coo_matrix(A)
        off = coo.row != coo.col
        assert np.all(colour_of[coo.row[off]] != colour_of[coo.col[off]])
        for d in ds:
            b = rng.standard_normal((A.shape[0], d)); x = rng.standard_normal((A.shape[0], d))
            for iters in (1, 2):
                got = eng.smooth(k, b, x, iters)
                want_p = oracle.gauss_seidel(Ap, b[order], x[order], iters)
                want = np.empty_like(want_p); want[order] = want_p
                assert rel(got, want) <= 1e-12


def timing_or_none(eng, key):
    """eng.timing(key), or None where the engine has no such key (yet): a key that only appears once its path has run.  Any other error
    is raised."""
    from gravo_mg_amd import cabi
    try:
        return eng.timing(key)
    except cabi.GmgError as e:
        if e.code == cabi.GMG_ERR_INVALID and "unknown timing key" in str(e):
            return None
        raise


def colour_permuted_hierarchy(P, eng, oracle, **kw):
    """The oracle on the device's colour ordering of every level (an engine with block_rows = 0): (oracle.Hierarchy of P A P^T with the permuted
    prolongations, the level-0 order).  kw goes to oracle.Hierarchy (pre_iters, post_iters)."""
    L = len(P.U)
    orders = []
    for k in range(L):
        n2o, _ = eng.level_ordering(k)
        orders.append(n2o[n2o >= 0])
    orders.append(np.arange(P.U[-1].shape[1]))
    Up = [sp.csc_matrix(sp.csc_matrix(P.U[k]).tocsr()[orders[k]][:, orders[k + 1]]) for k in range(L)]
    lhs_p = sp.csc_matrix(sp.csc_matrix(P.lhs).tocsr()[orders[0]][:, orders[0]])
    O = oracle.Hierarchy(Up, P.mass[orders[0]], **kw)
    O.set_system(lhs_p)
    return O, orders[0]


SWITCHES = ("speculate_head", "fuse_restrict_sweep", "uniform_slices", "fine_col16")


def engaged(eng, switch):
    """How much of the switched path ran, from the timing keys: heads enqueued ahead of the solve loop's decision, restrictions fused with
    the next level's first pre-sweep, level-0 operators with 16-bit column codes, the code width of those read as uniform slices."""
    def key(k):
        return timing_or_none(eng, k) or 0.0      # (keys that only appear once their path has been set up or run)
    if switch == "speculate_head":
        return key("heads_enqueued")
    if switch == "fuse_restrict_sweep":
        return key("restrict_sweeps_fused")
    ops = ("col16_l0", "col16_R_l0", "col16_P_l0")
    if switch == "fine_col16":
        return sum(key(k) for k in ops)
    return sum(key(k + "_uniform_width") for k in ops)
