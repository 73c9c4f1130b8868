"""CPU checks of the Kernel Inception Distance: the float64 restatement (tests/kid_ref.py) against an explicit double loop, the
error bound against the defects it must catch, the subset draws and estimator of autodiffusion_amd/kid.py with the restatement
standing in for the kernel, pooled_rows over two gloo ranks, the C ABI's refusals (argument checks run before any launch) and the
command lines' new flags."""
import importlib.util
import os
import socket

import numpy as np
import pytest
import torch

import kid_ref
from autodiffusion_amd import _lib, kid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_cli", os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _host_sums(monkeypatch):
    """kid.poly3_sums answered by the restatement on host tensors: everything of kid.py but the kernel call runs here."""
    monkeypatch.setattr(kid, "poly3_sums", lambda x, y=None: kid_ref.poly3_sum(x.numpy(), None if y is None else y.numpy())[0])


# ------------------------------------------------------------------ the restatement and its bound
def test_restatement_equals_the_double_loop():
    x, y = kid_ref.features(3, 8, 1), kid_ref.features(4, 8, 2)
    for a, b in ((x, y), (y, x), (x, None), (y, None)):
        s, sa = kid_ref.poly3_sum(a, b)
        assert s == pytest.approx(kid_ref.poly3_sum_loops(a, b), rel=1e-14)
        assert sa == pytest.approx(s, rel=1e-14)                    # non-negative rows: every k >= 1
    assert kid_ref.poly3_sum(x)[0] < kid_ref.poly3_sum(x, x)[0]     # the diagonal is left out
    assert kid_ref.mmd2_unbiased(x, y) == pytest.approx(kid_ref.mmd2_loops(x, y), rel=1e-12, abs=1e-15)
    # the reported KID: mean / std over draws made with one RandomState, sample set then reference set
    xs, ys = kid_ref.features(7, 8, 3), kid_ref.features(9, 8, 4)
    mean, std, vals = kid_ref.kid_subsets(xs, ys, subsets=3, subset_size=4, seed=5)
    rs = np.random.RandomState(5)
    want = []
    for _ in range(3):
        ix = rs.choice(7, 4, replace=False)
        iy = rs.choice(9, 4, replace=False)
        want.append(kid_ref.mmd2_loops(xs[ix], ys[iy]))
    np.testing.assert_allclose(vals, want, rtol=1e-12, atol=1e-15)
    assert mean == pytest.approx(np.mean(want)) and std == pytest.approx(np.std(want))


def test_mixed_sign_rows_have_negative_kernel_values():
    y = kid_ref.features(5, 36, 2, mixed_sign=True)
    x = kid_ref.oppose(kid_ref.features(4, 36, 1, mixed_sign=True), y)
    s, sa = kid_ref.poly3_sum(x, y)
    assert sa > s + 0.1 and kid_ref.kernel_matrix(x, y)[0, 0] < 0
    assert s == pytest.approx(kid_ref.poly3_sum_loops(x, y), rel=1e-13)


@pytest.mark.parametrize("n,m,d", [(65, 129, 36), (257, 130, 2048)])
def test_entrywise_bound_lies_below_the_stated_one_on_the_mixed_sign_sets(n, m, d):
    """The step of the derivation that mixed-sign rows do not grant entry by entry holds on the sum, on the sets the GPU test uses."""
    y = kid_ref.features(m, d, 12, mixed_sign=True)
    base = kid_ref.features(n, d, 11, mixed_sign=True)
    x = kid_ref.oppose(base, y)
    chain = kid.reduction_chain(n, m, False)
    assert kid_ref.bound_entrywise(x, y, chain) <= kid_ref.bound(kid_ref.poly3_sum(x, y)[1], d, chain)
    xs = kid_ref.oppose(base, base, 1, 0)
    assert kid_ref.poly3_sum(xs)[1] > kid_ref.poly3_sum(xs)[0] + 0.1
    chain = kid.reduction_chain(n, n, True)
    assert kid_ref.bound_entrywise(xs, xs, chain, True) <= kid_ref.bound(kid_ref.poly3_sum(xs)[1], d, chain)


def test_reduction_chain_restates_the_kernels_tree():
    assert kid.poly3_blocks(64, 64, False) == 1 and kid.poly3_blocks(65, 129, False) == 6 and kid.poly3_blocks(257, 257, True) == 15
    assert kid.reduction_chain(64, 64, False) == 16 + 6 + 3 + 1 + 8
    assert kid.reduction_chain(1, 1, False) == 1 and kid.reduction_chain(2, 3, False) == 6 and kid.reduction_chain(2, 2, True) == 2
    assert kid.reduction_chain(10000, 10000, True) == 16 + 6 + 3 + -(-(157 * 158 // 2) // 256) + 8
    lib = _lib.load()
    for n, m, sp in ((1, 1, 0), (65, 129, 0), (200, 1000, 0), (2, 2, 1), (257, 257, 1), (10000, 10000, 1), (50000, 50000, 0)):
        assert lib.adm_poly3_work_elems(n, m, sp) == kid.poly3_blocks(n, m, bool(sp)), (n, m, sp)
    for n, m in ((1, 1), (2, 3), (65, 129), (200, 1000)):     # never more than the pairs summed: adding a masked entry's exact 0.0 does not round
        assert kid.reduction_chain(n, m, False) <= n * m


def test_planted_defects_fall_outside_the_bound():
    n, m, d = 65, 129, 36
    x, y = kid_ref.features(n, d, 21), kid_ref.features(m, d, 22)
    for a, b, defects in ((x, y, ("padded_rows", "fp32_running_sum", "fp16_inputs")),
                          (y, None, ("diagonal_kept", "offdiag_once", "fp32_running_sum", "fp16_inputs"))):
        s, sa = kid_ref.poly3_sum(a, b)
        rows_b = len(a) if b is None else len(b)
        tol = kid_ref.bound(sa, d, kid.reduction_chain(len(a), rows_b, b is None))
        assert tol < 1e-12 * sa
        for defect in defects:
            bad = kid_ref.poly3_sum(a, b, defect)[0]
            assert abs(bad - s) > tol, (defect, abs(bad - s), tol)
        # a legitimate reordering stays inside: the transposed product, and float64 sums taken row by row
        k = kid_ref.kernel_matrix(a, a if b is None else b)
        if b is None:
            np.fill_diagonal(k, 0.0)
        assert abs(float(sum(float(r.sum()) for r in k.T)) - s) <= tol
    assert kid_ref.poly3_sum(x, y, "padded_rows")[0] - kid_ref.poly3_sum(x, y)[0] == pytest.approx(128 * 192 - 65 * 129, rel=1e-12)


# ------------------------------------------------------------------ kid.py around the kernel call
def test_kid_subsets_draw_order_and_short_sets(monkeypatch):
    _host_sums(monkeypatch)
    x, y = kid_ref.features(30, 8, 5), kid_ref.features(26, 8, 6) + 0.05
    mean, std = kid.kid_subsets(x, y, subsets=4, subset_size=10, seed=3)
    rmean, rstd, vals = kid_ref.kid_subsets(x.numpy(), y.numpy(), 4, 10, 3)
    assert mean == pytest.approx(rmean, rel=1e-10, abs=1e-14) and std == pytest.approx(rstd, rel=1e-10, abs=1e-14)
    draws = kid.draw_subsets(30, 26, 4, 10, 3)
    for (ix, iy), (jx, jy) in zip(draws, kid_ref.subset_draws(30, 26, 4, 10, 3)):
        assert np.array_equal(ix, jx) and np.array_equal(iy, jy)
    assert all(len(set(ix.tolist())) == 10 and len(set(iy.tolist())) == 10 for ix, iy in draws)   # without replacement
    swapped = kid.kid_subsets(y, x, subsets=4, subset_size=10, seed=3)[0]     # the draw order is part of the definition
    assert swapped != pytest.approx(mean, rel=1e-12)
    for a, b, which in ((x, y, "reference"), (y, x, "sample")):
        with pytest.raises(ValueError, match="--kid_subset_size") as e:
            kid.kid_subsets(a, b, subsets=2, subset_size=28)
        assert which in str(e.value) and "26" in str(e.value)
    assert kid.kid_subsets.__defaults__ == (100, 1000, 0)


def test_mmd2_unbiased_is_symmetric_and_matches_the_restatement(monkeypatch):
    _host_sums(monkeypatch)
    x, y = kid_ref.features(9, 12, 7), kid_ref.features(14, 12, 8) * 1.1
    a, b = kid.mmd2_unbiased(x, y), kid.mmd2_unbiased(y, x)
    assert a == pytest.approx(b, rel=1e-12, abs=1e-16) and a == pytest.approx(kid_ref.mmd2_unbiased(x.numpy(), y.numpy()), rel=1e-12)
    far = kid.mmd2_unbiased(x, y + 1.0)                                # an unbiased estimate may be negative; a shifted set is far
    assert far > 10 * abs(a) and far > 0
    assert kid.mmd2_unbiased(x, y, s_yy=kid_ref.poly3_sum(y.numpy())[0]) == a
    with pytest.raises(ValueError, match="at least 2 rows"):
        kid.mmd2_unbiased(x[:1], y)
    ref = kid.KIDReference.__new__(kid.KIDReference)     # the cached-S_yy path, without the constructor's device upload
    ref.y, ref.s_yy = y, kid_ref.poly3_sum(y.numpy())[0]
    assert ref.fitness(x) == pytest.approx(1000.0 * a, rel=1e-12)


def test_host_tensors_are_refused():
    x = kid_ref.features(4, 8, 1)
    with pytest.raises(_lib.AdmError, match="no CPU fallback"):
        kid.poly3_sums(x)
    with pytest.raises(_lib.AdmError, match="no CPU fallback"):
        kid.mmd2_unbiased(x, x)
    from autodiffusion_amd import ops
    with pytest.raises(_lib.AdmError):
        ops.poly3_sums(x, x)


def test_abi_refusals_need_no_gpu():
    """Every refusal is answered before anything is launched, so host placeholders stand in for the device buffers."""
    lib = _lib.load()
    X, Y, W, O = 0x10000, 0x20000, 0x30000, 0x40000
    ok = dict(x=X, n=65, y=Y, m=129, d=36, work=W, we=6, out=O, sp=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.adm_poly3_sums(a["x"], a["n"], a["y"], a["m"], a["d"], a["work"], a["we"], a["out"], None, a["sp"])
    cases = [(dict(x=None), -1, b"null"), (dict(y=None), -1, b"null"), (dict(work=None), -1, b"null"), (dict(out=None), -1, b"null"),
             (dict(n=0), -1, b"n >= 1"), (dict(m=0), -1, b"n >= 1"), (dict(m=-3), -1, b"n >= 1"),
             (dict(d=0), -2, b"multiple of 4"), (dict(d=2), -2, b"multiple of 4"), (dict(d=38), -2, b"multiple of 4"),
             (dict(we=5), -1, b"work holds 5"), (dict(sp=1), -1, b"self_pairs needs"), (dict(sp=1, y=None, m=65, we=2), -1, b"work holds 2"),
             (dict(sp=1, y=None), -1, b"m == n"), (dict(sp=2), -1, b"neither 0 nor 1"),
             (dict(x=X + 4), -3, b"16-byte"), (dict(y=Y + 8), -3, b"16-byte"), (dict(work=W + 4), -3, b"8-byte"), (dict(out=O + 4), -3, b"8-byte")]
    for kw, status, text in cases:
        assert call(**kw) == status and text in lib.adm_last_error(), (kw, lib.adm_last_error())
    assert lib.adm_poly3_work_elems(0, 5, 0) == -1 and lib.adm_poly3_work_elems(5, 6, 1) == -1
    sig = _lib.SIGNATURES["adm_poly3_sums"][1]
    assert sig[-1] is _lib._I and sig[-2] is _lib._P     # the stream is second to last: the symbol stays out of the replay census


# ------------------------------------------------------------------ pooled_rows over two gloo ranks
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _rank_rows(rank):
    return torch.arange(8 * 6, dtype=torch.float32).reshape(8, 6)[:5] if rank == 0 else torch.arange(8 * 6, dtype=torch.float32).reshape(8, 6)[5:]


def _rank_main(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mine = _rank_rows(rank)
    got = kid.pooled_rows(mine)
    local = kid.pooled_rows(mine, local=True)
    np.savez(out + str(rank) + ".npz", got=got.numpy(), local=local.numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_pooled_rows_two_ranks_gloo_with_unequal_counts(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / "rows")
    mp.spawn(_rank_main, args=(2, _free_port(), out), nprocs=2, join=True)
    want = torch.arange(8 * 6, dtype=torch.float32).reshape(8, 6).numpy()
    for rank in (0, 1):
        z = np.load(out + str(rank) + ".npz")
        assert np.array_equal(z["got"], want)                                   # 5 + 3 rows, in rank order, on both ranks
        assert np.array_equal(z["local"], _rank_rows(rank).numpy())
    x = torch.ones(3, 4)
    assert kid.pooled_rows(x) is x                                              # no process group: the rows as they are


# ------------------------------------------------------------------ the command lines
def test_parsers_accept_the_new_flags_and_default_to_fid():
    ev = _script("evaluator").create_argparser()
    a = ev.parse_args(["ref.npz", "smp.npz"])
    assert a.kid is False and (a.kid_subsets, a.kid_subset_size, a.kid_seed) == (100, 1000, 0) and a.save_ref_feats == ""
    a = ev.parse_args(["ref.npz", "smp.npz", "--kid", "True", "--kid_subsets", "3", "--kid_subset_size", "16", "--kid_seed", "9",
                       "--save_ref_feats", "f.npz"])
    assert a.kid is True and (a.kid_subsets, a.kid_subset_size, a.kid_seed, a.save_ref_feats) == (3, 16, 9, "f.npz")
    for name in ("search_ea", "sd_search_ea"):
        p = _script(name).create_argparser()
        a = p.parse_args([])
        assert a.fitness == "fid" and a.ref_feats == ""
        a = p.parse_args(["--fitness", "kid", "--ref_feats", "feats.npz"])
        assert a.fitness == "kid" and a.ref_feats == "feats.npz"
        with pytest.raises(SystemExit):
            p.parse_args(["--fitness", "mmd"])


def test_searchers_take_the_fitness_and_tag_their_lines(tmp_path):
    from types import SimpleNamespace
    from autodiffusion_amd import search
    from autodiffusion_amd.sd_evaluate import SDCandidateEvaluator
    feats = str(tmp_path / "feats.npz")
    np.savez(feats, feats=kid_ref.features(6, 8, 1).numpy())
    args = SimpleNamespace(max_epochs=1, select_num=2, population_num=3, m_prob=0.25, crossover_num=1, mutation_num=1)
    feat_fn = lambda u8: u8     # noqa: E731
    s = search.EvolutionSearcher(args, None, None, 4, features=feat_fn)
    assert s.fitness == "fid" and s.fid_note == "" and s.kid_ref is None
    args.fitness, args.ref_feats = "kid", feats
    s = search.EvolutionSearcher(args, None, None, 4, features=feat_fn)
    assert s.fitness == "kid" and s.fid_note == " [fitness: KID x 1e3]" and s._ref_feats.shape == (6, 8) and s._ref_feats.dtype == np.float32
    args.ref_feats = ""
    with pytest.raises(ValueError, match="--ref_feats"):
        search.EvolutionSearcher(args, None, None, 4, features=feat_fn)
    args.fitness = "mmd"
    with pytest.raises(ValueError, match="'fid' or 'kid'"):
        search.EvolutionSearcher(args, None, None, 4, features=feat_fn)
    with pytest.raises(KeyError, match="feats"):
        np.savez(str(tmp_path / "stats.npz"), mu=np.zeros(3))
        kid.load_ref_feats(str(tmp_path / "stats.npz"))
    e = SDCandidateEvaluator(None, None, conditioning=[], num_samples=4, features=feat_fn, fitness="kid", ref_feats=feats, device="cpu")
    assert e.fid_note == " [fitness: KID x 1e3]" and e.ref_stats is None and e._accumulator().keep_rows > 4
    e = SDCandidateEvaluator(None, None, conditioning=[], ref_mu=np.zeros(4), ref_sigma=np.eye(4), num_samples=4, features=feat_fn, device="cpu")
    assert e.fitness == "fid" and e.fid_note == "" and e._accumulator().rows is None
    with pytest.raises(ValueError, match="ref_feats"):
        SDCandidateEvaluator(None, None, conditioning=[], num_samples=4, features=feat_fn, fitness="kid", device="cpu")
