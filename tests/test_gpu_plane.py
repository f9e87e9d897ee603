"""GPU: gsx_model_fit_plane and gsx_model_select_plane (spec/RENDER_SPEC.md §28; csrc/kernels_plane.hip).  The yardsticks:
gsx_model_download_pod for the stored positions, the float32 definition tests/plane_ref.py (tests/test_plane_cpu.py ties it to
csrc/plane_math.h), the sanitized host driver tests/plane_driver.cpp for the candidates and the solve, tests/extract_ref.py for the
filter.  Counts, candidates, the winner, every selection word and the solve are compared bit for bit; the moments within the derived
bound of a reordered float64 sum (tests/test_plane_cpu.py: assert_moments_within_bound).
Sizes: a workgroup takes chunks of 1024 Gaussians in four rounds of 256, a wave 64 of them; the score's grid is capped at 2048
workgroups and the moments' finish has 256 lanes: one Gaussian, a wave edge (63, 64, 65), a round edge (255, 256, 257), a chunk edge
(1023, 1024, 1025), chunks with a partial last one (2049, 5000), 257 * 1024 + 1: 258 partials, a second round of the finish's lanes,
and 2048 * 1024 + 1025: 2050 chunks, so that workgroups of the capped grids take a second chunk.  Candidates: one, a wave of
counters and its edges (63, 64, 65), several waves (256) and the most (1024).
The level tolerance (test_level_stands_the_lattice_up): measured on the CPU path — plane_ref.fit of the tilted lattice, plane_ref.level,
the float32 quat and pos applied by tests/transform_ref.py's float32 formula, plane_ref.fit again — the refitted normal was 1.96e-8
from up in its worst component (the float32 roundings of the moved positions, 8.9e-8 off the floor at most, against an extent of 1);
asserted 16 x that."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import common
from tests import extract_ref as X
from tests import plane_ref as PR
from tests import transform_ref as T
from tests.model_ops import H as FB_H, KIND_IDS, KINDS, W as FB_W, frames as _frames, load as _load, pod as _pod
from tests.test_gpu_knn import _filter_model, _points_model
from tests.test_plane_cpu import assert_moments_within_bound, assert_peel, build_driver, play_fit, play_solve
from wgpu_3dgs_viewer_app_amd import _lib
from wgpu_3dgs_viewer_app_amd import viewer as viewer_mod
from wgpu_3dgs_viewer_app_amd.viewer import CommGroup, GsxError, MultiModelViewer, ShKind, plane_level

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5000]
BIG = 257 * 1024 + 1
LEVEL_TOL = 16 * 1.96e-8
INF = float("inf")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("plane_gpu"))


@pytest.fixture(scope="module")
def corner():
    """seed -> (pos, normals, variation) of the 3000-point corner, made once and not changed"""
    return {seed: PR.corner(seed) for seed in range(3)}


def _cloud(n, seed):
    """n points: a third of them within 0.01 of the plane x + 2y - z = 0.3 (not axis aligned), the rest in the unit box"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3))
    on = rng.random(n) < 0.34
    p[on, 2] = p[on, 0] + 2 * p[on, 1] - 0.3 + rng.normal(0, 0.004, int(on.sum()))
    return p.astype(F)


def _caller_planes(H, seed):
    """H planes that are not axis aligned, most of them near x + 2y - z = 0.3 normalised, not all of unit length"""
    rng = np.random.default_rng(seed)
    n = np.array([1.0, 2.0, -1.0]) / math.sqrt(6.0) + rng.normal(0, 0.02, (H, 3))
    n[::7] *= 1.5
    return np.concatenate([n, (0.3 / math.sqrt(6.0) + rng.normal(0, 0.01, H))[:, None]], axis=1).astype(F)


def _check_counts(got, pos, part, tolerance, min_cos=0.0, normals=None, variation=None, what=""):
    """out_counts against the brute-force float32 answer computed from the device's own out_candidates"""
    valid = np.any(got.candidates != 0, axis=1)  # (an invalid candidate is reported as zeros, and only such a one)
    want = PR.counts(got.candidates, valid, pos, part, tolerance, min_cos, normals, variation)
    assert np.array_equal(got.counts, want), what
    assert got.n_valid == int(valid.sum()) and got.count == int(part.sum()), what
    w = PR.winner(want, valid)
    assert (got.winner if got.winner is not None else PR.NONE) == w, what
    if w != PR.NONE:
        assert got.candidate_inliers == int(want[w]), what
    return want, valid


# ---- 1. the score, exact ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_counts_are_the_brute_force_answer(n):
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, _cloud(n, 100 + n))
        part = PR.participants(pos)
        for H in ((1, 64, 1024) if n in (1, 257, 5000) else (63, 65) if n in (64, 1024) else (256,)):
            for sample in (PR.TRIPLES, PR.CALLER):
                given = _caller_planes(H, n + H) if sample == PR.CALLER else None
                got = m.fit_plane(0.01, H, sample, seed=n * 7 + H, refine_iters=0, candidates=given)
                _check_counts(got, pos, part, 0.01, what=(n, H, sample))
                if sample == PR.CALLER:
                    assert got.candidates.tobytes() == given.tobytes() and got.n_valid == H  # used as given: not normalised


def test_moments_over_more_partials_than_the_finish_has_lanes(driver):
    """257 * 1024 + 1 Gaussians: 258 chunks, 258 partials of the moments, so that lanes of the one-workgroup finish take a second one.
    Every participant is an inlier of the caller's plane (the tolerance spans the cloud), so the round is accepted: the moments
    against the exactly summed reference, the solve the driver's bit for bit.  The counts exact at this size too."""
    n = BIG
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, _cloud(n, 9))
        part = PR.participants(pos)
        got = m.fit_plane(10.0, candidates=F([[1 / 3, 2 / 3, -2 / 3, 0.1]]), refine_iters=1)
        assert got.candidate_inliers == n == got.n_inliers
        _check_refine_round(driver, got, pos, part, 10.0, accepted=True)
        given = _caller_planes(65, 3)
        got = m.fit_plane(0.01, candidates=given, refine_iters=1)
        want, _ = _check_counts(got, pos, part, 0.01)
        assert want.max() > 256 * 1024 * 0.2 and got.n_inliers >= got.candidate_inliers
        _check_refine_round(driver, got, pos, part, 0.01, accepted=False)  # (by the reference 92938 inliers would become 92908)
        some = m.fit_plane(0.01, 256, seed=5, refine_iters=0)
        _check_counts(some, pos, part, 0.01)


def test_a_workgroup_takes_a_second_chunk():
    """The grids of the participants', the score's and the select's kernels are capped at 2048 workgroups: past 2048 x 1024 Gaussians a
    workgroup strides over several chunks, carries its LDS counters across them and reloads the Gaussians it holds in registers.
    2048 * 1024 + 1025 Gaussians (tests/test_gpu_property.py's size), the planes staged on the device: count and n_nonfinite, the
    counts without and with min_cos exact, select_plane's words."""
    import torch

    n = 2048 * 1024 + 1025
    rng = np.random.default_rng(9)
    pos = _cloud(n, 19)
    pos[[0, n // 2, n - 1], 0] = [np.nan, np.inf, -np.inf]
    color = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    cov = np.zeros((n, 6), F)
    cov[:, 0] = cov[:, 3] = cov[:, 5] = F(1e-4)
    mask = rng.random(n) < 0.5
    given = _caller_planes(17, 5)  # (few planes: the reference takes 30 ms a plane at this size)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        v.add_model("src", n)
        m = v.models["src"]
        dev = [torch.from_numpy(a).cuda() for a in (pos, color.view(np.int32), cov)]
        torch.cuda.synchronize()
        m.gaussian_buffers.gaussians_buffer.update_range_pod_device(0, n, dev[0].data_ptr(), dev[1].data_ptr(), None, dev[2].data_ptr())
        v.poll()
        m.gaussian_buffers.mask_buffer.upload(X.words(mask, True))
        assert _pod(v)[0].tobytes() == pos.tobytes()
        fin = PR.participants(pos)
        got = m.fit_plane(0.01, candidates=given, refine_iters=0)
        assert (got.count, got.n_nonfinite) == (n - 3, 3)
        _check_counts(got, pos, fin, 0.01)
        masked = m.fit_plane(0.01, candidates=given[:9], refine_iters=0, filter=X.MASKED)
        assert (masked.count, masked.n_nonfinite) == (int((fin & mask).sum()), int((~fin & mask).sum()))
        _check_counts(masked, pos, fin & mask, 0.01)
        m.keep_normals(8)
        kept = m.kept_normals()
        facing = m.fit_plane(0.01, candidates=given[:9], refine_iters=0, min_cos=0.5)
        want, _ = _check_counts(facing, pos, fin, 0.01, 0.5, kept.normal, kept.variation)
        assert 0 < want.max() < got.counts[:9].max()
        plane = given[int(np.argmax(got.counts))]
        hit = PR.in_range(plane, pos, fin & mask, -0.01, INF)
        assert m.select_plane(plane, -0.01, INF, filter=X.MASKED) == (int(hit.sum()), int(hit.sum()))
        assert np.array_equal(m.gaussian_buffers.selection_buffer.download(), X.words(hit))
        hit2 = PR.in_range(plane, pos, fin, -0.01, 0.01, 0.5, kept.normal, kept.variation)
        assert m.select_plane(plane, -0.01, 0.01, min_cos=0.5, op=_lib.GSX_SELECTION_ADD) == (int(hit2.sum()), int((hit | hit2).sum()))
        assert np.array_equal(m.gaussian_buffers.selection_buffer.download(), X.words(hit | hit2))


def _check_refine_round(driver, got, pos, part, tolerance, accepted, min_cos=0.0, normals=None, variation=None, toward=None):
    """A fit asked for one refine round.  accepted=True: the round must have been accepted; its sums against the reference over the
    candidate's inliers, the solve against the driver's on the device's own sums bit for bit, the recount.  accepted=False: it must
    have been refused, and the reference's round loses inliers too.  accepted=None: the caller does not know; whichever happened is
    checked in its way."""
    inl = PR.inliers(got.candidate, pos, part, tolerance, min_cos, normals, variation)
    ref = PR.moments(got.candidate, pos, inl)
    assert ref["count"] == got.candidate_inliers and got.refine_done in (0, 1)
    if accepted is not None:
        assert got.refine_done == (1 if accepted else 0)
    if got.refine_done == 0:
        f = PR.solve(ref, toward)
        assert f is None or int(PR.inliers(f["plane"], pos, part, tolerance, min_cos, normals, variation).sum()) < got.candidate_inliers
        assert got.plane.tobytes() == got.candidate.tobytes() and got.n_inliers == got.candidate_inliers and not got.sums.any()
        return
    assert_moments_within_bound(dict(count=got.candidate_inliers, sum_p=got.sums[0:3], scatter=got.sums[3:9]), ref)
    solved = play_solve(driver, got.candidate_inliers, got.sums[0:3], got.sums[3:9], toward)
    assert solved["ok"] and solved["plane"].tobytes() == got.plane.tobytes() and solved["centre"].tobytes() == got.centroid.tobytes()
    assert np.array_equal(solved["eigenvalues"], got.eigenvalues)
    again = PR.inliers(got.plane, pos, part, tolerance, min_cos, normals, variation)
    assert got.n_inliers == int(again.sum()) >= got.candidate_inliers
    nxt = PR.moments(got.plane, pos, again)
    assert abs(got.sums[9] - nxt["sum_r2"]) <= PR.bound(nxt["count"], nxt["mag"]["sum_r2"])
    assert got.rms == math.sqrt(got.sums[9] / got.n_inliers)


# ---- 2. the boundary -----------------------------------------------------------------------------------------------------------------------
def test_the_bound_is_inclusive_on_a_dyadic_lattice():
    """Coordinates, offsets and tolerances are multiples of 2^-8 below 2, the planes are axis-aligned unit planes: every residual is exact."""
    step = 2.0 ** -8
    side = 17
    u = (np.arange(side) - 8) * step * 4  # -32 .. 32 steps
    pos = np.stack(np.meshgrid(u, u, u, indexing="ij"), axis=-1).reshape(-1, 3).astype(F)
    n = len(pos)
    holes = pos.copy()
    holes[3, 0], holes[side * side * 8 + 5, 2], holes[n - 1, 1], holes[100, 1] = np.nan, np.inf, -np.inf, np.nan
    planes = F([[1, 0, 0, 0], [0, 1, 0, 4 * step], [0, 0, 1, -8 * step], [0, -1, 0, 12 * step]])
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, stored = _points_model(v, holes)
        assert np.array_equal(np.isfinite(stored), np.isfinite(holes))
        part = PR.participants(stored)
        assert int((~part).sum()) == 4
        for k in (0, 1, 2, 3):  # tolerance k * 4 steps: the lattice layers at exactly that distance count, the next ones do not
            tol = k * 4 * step
            got = m.fit_plane(tol, candidates=planes, refine_iters=0)
            assert (got.count, got.n_nonfinite) == (n - 4, 4)
            for h, (axis, off) in enumerate(((0, 0.0), (1, 4 * step), (2, -8 * step), (1, -12 * step))):
                d = np.abs(stored[:, axis].astype(np.float64) - off)
                want = int((part & (d <= tol)).sum())
                assert got.counts[h] == want and int((part & (d <= tol + 4 * step)).sum()) > want  # (one lattice step out is not counted)
                assert int((part & (d == tol)).sum()) > 0  # (there are points exactly on the bound)
            _check_counts(got, stored, part, tol)
        zero = m.fit_plane(0.0, candidates=planes, refine_iters=0)
        assert zero.counts[0] == int((part & (stored[:, 0] == 0)).sum()) > 0  # tolerance 0: the coplanar points only


# ---- 3. the candidates ------------------------------------------------------------------------------------------------------------------------
def test_candidates_are_the_drivers_bit_for_bit(driver, corner):
    pos0, nrm, var = corner[0]
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, pos0)
        n = len(pos)
        m.keep_normals(8)
        kept = m.kept_normals()
        part = PR.participants(pos)
        for sample, H, seed in ((PR.TRIPLES, 256, 7), (PR.NORMALS, 256, 7), (PR.TRIPLES, 65, 2 ** 64 - 3), (PR.NORMALS, 1, 0)):
            got = m.fit_plane(0.006, H, sample, seed=seed, refine_iters=0)
            want = play_fit(driver, pos, part, sample, H, seed, 0.006, normals=kept.normal, variation=kept.variation)
            assert got.candidates.tobytes() == want["planes"].tobytes() and np.array_equal(got.counts, want["counts"]), (sample, H)
            assert got.winner == want["winner"] and got.n_valid == int(want["valid"].sum()) == H
            _, _, slots = PR.candidates(pos, part, sample, H, seed, kept.normal, kept.variation)
            assert np.array_equal(want["slots"], slots & 0xFFFFFFFF)  # the sampled indices: the reference's
            again = m.fit_plane(0.006, H, sample, seed=seed, refine_iters=0)
            assert again.candidates.tobytes() == got.candidates.tobytes() and again.counts.tobytes() == got.counts.tobytes()
            other = m.fit_plane(0.006, H, sample, seed=seed ^ 1, refine_iters=0)
            assert other.candidates.tobytes() != got.candidates.tobytes()
        # a filter that leaves one Gaussian in three still yields every candidate valid
        third = np.arange(n) % 3 == 0
        m.gaussian_buffers.selection_buffer.upload(X.words(third, True))
        for sample in (PR.TRIPLES, PR.NORMALS):
            got = m.fit_plane(0.006, 256, sample, seed=13, refine_iters=0, filter=X.SELECTED)
            want = play_fit(driver, pos, part & third, sample, 256, 13, 0.006, normals=kept.normal, variation=kept.variation)
            assert got.n_valid == 256 and got.count == int(third.sum()) and got.candidates.tobytes() == want["planes"].tobytes()
            assert np.array_equal(got.counts, want["counts"])
            inv = m.fit_plane(0.006, 64, sample, seed=11, refine_iters=0, filter=X.SELECTED, invert=True)  # the peel's filter
            want = play_fit(driver, pos, part & ~third, sample, 64, 11, 0.006, normals=kept.normal, variation=kept.variation)
            assert inv.count == int((~third).sum()) and inv.candidates.tobytes() == want["planes"].tobytes() and np.array_equal(inv.counts, want["counts"])
        # fewer than three participants: no triple, the call is degenerate and GSX_OK
        for keep in (0, 1, 2):
            m.gaussian_buffers.selection_buffer.upload(X.words(np.arange(n) < keep, True))
            got = m.fit_plane(0.006, 64, PR.TRIPLES, seed=3, filter=X.SELECTED)
            assert got.degenerate and got.n_valid == 0 and got.winner is None and got.count == keep and not got.plane.any() and not got.counts.any()
            assert not got.candidates.any() and (got.n_inliers, got.candidate_inliers, got.refine_done, got.rms) == (0, 0, 0, 0.0)
        # a valid winner with fewer than three inliers is no plane either
        far = m.fit_plane(0.006, candidates=F([[0, 0, 1, 50.0], [0, 1, 0, -50.0]]))
        assert far.degenerate and far.n_valid == 2 and far.winner == 0 and far.candidate_inliers == 0 and not far.plane.any() and not far.candidate.any()
        assert far.candidates.tobytes() == F([[0, 0, 1, 50.0], [0, 1, 0, -50.0]]).tobytes()


# ---- 4. min_cos ----------------------------------------------------------------------------------------------------------------------------------
def test_min_cos_counts_and_refusal(corner):
    pos0, _, _ = corner[1]
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, pos0)
        part = PR.participants(pos)
        with pytest.raises(GsxError, match="gsx_model_normals_keep") as e:
            m.fit_plane(0.006, min_cos=0.9)
        assert e.value.status == _lib.GSX_ERR_INVALID_ARG
        with pytest.raises(GsxError, match="gsx_model_normals_keep") as e:
            m.fit_plane(0.006, sample=PR.NORMALS)
        assert e.value.status == _lib.GSX_ERR_INVALID_ARG
        with pytest.raises(GsxError, match="gsx_model_normals_keep") as e:
            m.select_plane([0, 0, 1, 0], -1, 1, min_cos=0.5)
        assert e.value.status == _lib.GSX_ERR_INVALID_ARG
        m.gaussian_buffers.selection_buffer.upload(X.words(np.arange(len(pos)) % 5 != 0, True))
        m.keep_normals(8, filter=X.SELECTED)  # every fifth Gaussian has no plane
        kept = m.kept_normals()
        assert 0 < kept.n_fitted < len(pos)
        for sample, H in ((PR.TRIPLES, 256), (PR.NORMALS, 65)):
            plain = m.fit_plane(0.006, H, sample, seed=7, refine_iters=0)
            got = m.fit_plane(0.006, H, sample, seed=7, refine_iters=0, min_cos=0.95)
            assert got.candidates.tobytes() == plain.candidates.tobytes()
            want, valid = _check_counts(got, pos, part, 0.006, 0.95, kept.normal, kept.variation)
            # ... and the counts without min_cos minus exactly the reference's rejected rows
            for h in range(H):
                near = PR.inliers(plain.candidates[h], pos, part, 0.006)
                rejected = near & ~PR.facing(plain.candidates[h], kept.normal, kept.variation, 0.95)
                assert plain.counts[h] - got.counts[h] == int(rejected.sum())
            assert (plain.counts > got.counts).any()
        one = m.fit_plane(0.006, 64, seed=7, refine_iters=0, min_cos=1.0)  # (1 is legal: only kept normals that are the plane's own)
        _check_counts(one, pos, part, 0.006, 1.0, kept.normal, kept.variation)


# ---- 5. moments and refine ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 64, 65, 256, 257, 1024, 1025, 5000])
def test_moments_and_the_solve(driver, n):
    """every participant is an inlier of the caller's plane (the tolerance spans the cloud): the inlier counts sit at the pass edges"""
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, _cloud(n, 40 + n))
        part = PR.participants(pos)
        plane = F([[1 / 3, 2 / 3, -2 / 3, 0.1]])
        for toward in (None, (0.5, 0.5, 5.0)):
            got = m.fit_plane(10.0, candidates=plane, refine_iters=1, toward=toward)
            assert got.candidate_inliers == n == got.n_inliers and got.refine_done == 1 and not got.degenerate
            _check_refine_round(driver, got, pos, part, 10.0, accepted=True, toward=toward)
        # a sampled winner at the working tolerance: whether its round is accepted depends on the sample (by the reference it is at the
        # small sizes and is not from 257 on); an accepted round is held to the driver, a refused one to the reference's own loss
        tight = m.fit_plane(0.01, 256, seed=n, refine_iters=1)
        assert not tight.degenerate and tight.n_inliers >= tight.candidate_inliers >= 3
        _check_refine_round(driver, tight, pos, part, 0.01, accepted=None)


def test_refine_follows_the_reference_and_its_stop_rule(driver, corner):
    """tests/test_plane_cpu.py's stop-rule fixture (corner seed 2, NORMALS, 256 candidates, seed 7, tolerance 0.006): the second round
    would lose an inlier (1036 -> 1035), so the call keeps the first round's plane whatever refine_iters asks for."""
    pos0, _, _ = corner[2]
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, pos0)
        m.keep_normals(8)
        kept = m.kept_normals()
        part = PR.participants(pos)
        ref = PR.fit(pos, part, PR.NORMALS, 256, 7, 0.006, refine_iters=4, normals=kept.normal, variation=kept.variation)
        assert ref["history"][-1] < ref["n_inliers"] and ref["refine_done"] == len(ref["history"]) - 1 >= 1  # (the fixture still stops)
        for iters in (0, 1, 2, 4, 8):
            got = m.fit_plane(0.006, 256, PR.NORMALS, seed=7, refine_iters=iters)
            want = PR.fit(pos, part, PR.NORMALS, 256, 7, 0.006, refine_iters=iters, normals=kept.normal, variation=kept.variation)
            assert (got.winner, got.candidate_inliers, got.n_inliers, got.refine_done) == (want["winner"], want["candidate_inliers"], want["n_inliers"], want["refine_done"])
            assert got.n_inliers >= got.candidate_inliers and got.candidate.tobytes() == want["candidate"].tobytes()
            assert np.abs(got.plane.astype(np.float64) - want["plane"]).max() <= 3 * 2.0 ** -23  # (numpy's eigh: test_plane_cpu.py's bound)
            if got.refine_done:
                assert abs(got.rms - want["rms"]) <= 1e-9 and got.rms == math.sqrt(got.sums[9] / got.n_inliers)
                again = m.fit_plane(0.006, 256, PR.NORMALS, seed=7, refine_iters=iters)  # the same bits every call
                assert again.plane.tobytes() == got.plane.tobytes() and again.sums.tobytes() == got.sums.tobytes() and again.rms == got.rms
            else:
                assert got.plane.tobytes() == got.candidate.tobytes() and got.rms == 0 and not got.sums.any() and not got.eigenvalues.any()


# ---- 6. the peel on the device --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", [PR.TRIPLES, PR.NORMALS])
def test_three_fits_peel_the_corner(corner, sample):
    for seed, (pos0, _, _) in corner.items():
        with MultiModelViewer(sh=ShKind.Remove) as v:
            m, pos = _points_model(v, pos0)
            if sample == PR.NORMALS:
                m.keep_normals(8)
            planes, n_inliers, taken = [], [], np.zeros(len(pos), bool)
            for call in range(3):
                got = m.fit_plane(0.006, 256, sample, seed=7, refine_iters=2, filter=X.SELECTED, invert=True)
                assert not got.degenerate and got.count == int((~taken).sum()) and got.n_inliers >= got.candidate_inliers
                hit, selected = m.select_plane(got.plane, -0.006, 0.006, op=_lib.GSX_SELECTION_ADD, filter=0)
                inl = PR.inliers(got.plane, pos, ~taken, 0.006)
                assert got.n_inliers == int(inl.sum())
                taken |= PR.inliers(got.plane, pos, np.ones(len(pos), bool), 0.006)
                assert selected == int(taken.sum()) and np.array_equal(X.bits(m.gaussian_buffers.selection_buffer.download(), len(pos)), taken)
                planes.append(got.plane)
                n_inliers.append(got.n_inliers)
            assert_peel(planes, n_inliers, seed)


# ---- 7. select_plane -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 2500])
def test_select_plane_every_op_range_and_filter(n):
    with MultiModelViewer(sh=ShKind.Remove) as v:
        g, mask, sel, flags = _filter_model(v, n, 500 + n)
        m = v.models["src"]
        pos = _pod(v)[0]
        fin = PR.participants(pos)
        sb = m.gaussian_buffers.selection_buffer
        plane = F([0.6, 0.0, 0.8, 0.1])
        now = sel.copy()
        ranges = ((-0.2, 0.3), (0.0, INF), (-INF, 0.05), (-INF, INF), (0.25, 0.25))
        for flt in (0, X.MASKED, X.SKIP_HIDDEN, X.SELECTED, 7):
            for op in (_lib.GSX_SELECTION_SET, _lib.GSX_SELECTION_ADD, _lib.GSX_SELECTION_REMOVE):
                lo, hi = ranges[(flt + op) % len(ranges)]
                passes = np.zeros(n, bool)
                passes[X.kept(n, flt, 0, mask, now, flags)] = True  # (SELECTED reads the selection as it was before the call)
                want = PR.in_range(plane, pos, fin & passes, lo, hi)
                after = want if op == _lib.GSX_SELECTION_SET else (now | want) if op == _lib.GSX_SELECTION_ADD else (now & ~want)
                assert m.select_plane(plane, lo, hi, op=op, filter=flt) == (int(want.sum()), int(after.sum())), (flt, op)
                assert np.array_equal(sb.download(), X.words(after)), (flt, op)  # (the tail bits are cleared)
                now = after
        assert int(PR.in_range(plane, pos, fin, -INF, INF).sum()) == int(fin.sum()) < n  # (a Gaussian without a finite position is never hit)
    with MultiModelViewer(sh=ShKind.Remove) as v:  # a model without a selection
        m, pos = _points_model(v, _cloud(n, 5))
        want = PR.in_range(F([0, 0, 1, 0.5]), pos, PR.participants(pos), 0.0, INF)
        assert m.select_plane([0, 0, 1, 0.5], 0.0, INF, op=_lib.GSX_SELECTION_REMOVE) == (int(want.sum()), 0)
        assert m.select_plane([0, 0, 1, 0.5], 0.0, INF, filter=X.SELECTED) == (0, 0)  # none selected = none pass
        assert m.select_plane([0, 0, 1, 0.5], 0.0, INF, op=_lib.GSX_SELECTION_ADD) == (int(want.sum()), int(want.sum()))
        assert np.array_equal(m.gaussian_buffers.selection_buffer.download(), X.words(want))


def test_select_plane_after_a_fit_hits_the_inliers(corner):
    pos0, _, _ = corner[0]
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, pos0)
        m.keep_normals(8)
        kept = m.kept_normals()
        for min_cos in (0.0, 0.9):
            fit = m.fit_plane(0.006, 256, seed=7, refine_iters=2, min_cos=min_cos)
            hit, selected = m.select_plane(fit.plane, -0.006, 0.006, min_cos=min_cos)
            assert hit == selected == fit.n_inliers
            want = PR.inliers(fit.plane, pos, PR.participants(pos), 0.006, min_cos, kept.normal, kept.variation)
            assert np.array_equal(m.gaussian_buffers.selection_buffer.download(), X.words(want))
        # remove the floor: everything at or below the plane's band, then the rest extracted
        fit = m.fit_plane(0.006, 256, seed=7)
        hit, _ = m.select_plane(fit.plane, -INF, 0.006)
        m.extract("rest", X.SELECTED, invert=True)
        assert v.models["rest"].gaussian_buffers.gaussians_buffer.len() == len(pos) - hit
        assert (PR.residual(fit.plane, _pod(v, "rest")[0]) > F(0.006)).all()


def test_select_plane_over_258_chunks():
    n = BIG
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, _cloud(n, 9))
        plane = F([1, 2, -1, 0.3]) / F(math.sqrt(6.0))
        want = PR.in_range(plane, pos, PR.participants(pos), -0.01, 0.01)
        assert m.select_plane(plane, -0.01, 0.01) == (int(want.sum()), int(want.sum()))
        assert np.array_equal(m.gaussian_buffers.selection_buffer.download(), X.words(want))


# ---- 8. level -----------------------------------------------------------------------------------------------------------------------------------------
def test_level_stands_the_lattice_up():
    pos0, normal = PR.tilted_lattice()
    up = (0.0, 0.0, 1.0)
    # the CPU path, which the tolerance was measured on
    part = PR.participants(pos0)
    ref = PR.fit(pos0, part, PR.TRIPLES, 64, 1, 1e-4, refine_iters=2, toward=(0, 0, 100))
    q, t = PR.level(ref["plane"], up)
    moved = T.position(pos0, t.astype(F), q.astype(F), (1, 1, 1))
    again = PR.fit(moved, part, PR.TRIPLES, 64, 1, 1e-4, refine_iters=2, toward=(0, 0, 100))
    cpu_dev = np.abs(again["plane"][:3].astype(np.float64) - up).max()
    print(f"CPU path: refitted normal {cpu_dev:.2e} from up, offset {again['plane'][3]:.2e}")
    assert cpu_dev <= LEVEL_TOL
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, pos0)
        fit = m.fit_plane(1e-4, 64, seed=1, refine_iters=2, toward=(0, 0, 100))
        assert fit.n_inliers == len(pos) and np.abs(fit.plane[:3].astype(np.float64) - normal).max() <= 3 * 2.0 ** -23 + 1e-7
        quat, t = plane_level(fit.plane, up)
        assert m.apply_transform(pos=tuple(t), quat=tuple(quat)) == len(pos)
        m = v.models["src"]
        fit2 = m.fit_plane(1e-4, 64, seed=1, refine_iters=2, toward=(0, 0, 100))
        dev = np.abs(fit2.plane[:3].astype(np.float64) - up).max()
        print(f"device: refitted normal {dev:.2e} from up, offset {fit2.plane[3]:.2e}")
        assert fit2.n_inliers == len(pos) and dev <= LEVEL_TOL and abs(float(fit2.plane[3])) <= 1e-6  # the floor at height 0
        assert np.abs(_pod(v)[0][:, 2]).max() <= 1e-6


# ---- 9. surroundings -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_every_pod_kind(kind):
    sh, cov = kind
    g = common.small_scene(1500, 77, 0)
    g["pos"] = _cloud(1500, 77)
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, g)
        m = v.models["src"]
        pos = _pod(v)[0]
        part = PR.participants(pos)
        got = m.fit_plane(0.01, 65, seed=4, refine_iters=1)
        _check_counts(got, pos, part, 0.01)
        want = PR.in_range(got.plane, pos, part, -0.01, 0.01)
        assert m.select_plane(got.plane, -0.01, 0.01) == (int(want.sum()), int(want.sum())) and int(want.sum()) == got.n_inliers


def test_nothing_a_frame_reads_is_written_and_the_workspace_is_steady(corner):
    pos0, _, _ = corner[0]
    before = viewer_mod.device_bytes()
    with MultiModelViewer() as v, MultiModelViewer() as twin:
        g = common.small_scene(len(pos0), 5, 3)
        g["pos"] = pos0
        _load(v, g)
        _load(twin, g)
        m = v.models["src"]
        sel = np.arange(len(pos0)) % 4 == 0
        m.gaussian_buffers.selection_buffer.upload(X.words(sel))
        m.keep_normals(8)
        kept = m.kept_normals()
        state = lambda: (tuple(a.tobytes() for a in m.gaussian_buffers.gaussians_buffer.download_pod()), m.gaussian_buffers.selection_buffer.download().tobytes())  # noqa: E731
        start = state()
        twin.models["src"].gaussian_buffers.selection_buffer.upload(X.words(sel))
        assert np.array_equal(_frames(v, ["src"], poses=(5,))[0], _frames(twin, ["src"], poses=(5,))[0])
        m.fit_plane(0.006, 1024, seed=1, refine_iters=8)  # (the first call sizes the workspace)
        held = viewer_mod.device_bytes()
        for kw in (dict(sample=PR.NORMALS), dict(min_cos=0.9), dict(filter=X.SELECTED), dict(n_candidates=1), dict(candidates=F([[0, 0, 1, 0]]))):
            m.fit_plane(0.006, **{"n_candidates": 256, "seed": 3, **kw})
        assert viewer_mod.device_bytes() == held  # the documented workspace: it stays with the viewer, as the other model operations'
        assert state() == start
        after = m.kept_normals()
        assert after.present and after.normal.tobytes() == kept.normal.tobytes() and after.variation.tobytes() == kept.variation.tobytes()
        for a, b in zip(_frames(v, ["src"], poses=(6, 7)), _frames(twin, ["src"], poses=(6, 7))):  # a frame after is the twin's, byte for byte
            assert np.array_equal(a, b)
        m.select_plane([0, 0, 1, 0], -0.01, 0.01, op=_lib.GSX_SELECTION_ADD)
        assert tuple(a.tobytes() for a in m.gaussian_buffers.gaussians_buffer.download_pod()) == start[0]
        assert m.kept_normals().normal.tobytes() == kept.normal.tobytes()
    assert viewer_mod.device_bytes() == before  # released with the viewer


def test_refusals_and_empty_models():
    g = common.small_scene(200, 3, 0)
    with MultiModelViewer(sh=ShKind.Remove) as v, MultiModelViewer(sh=ShKind.Remove) as other:
        _load(v, g)
        m = v.models["src"]
        L, h = v._L, v._h
        INV, NF, UNS = _lib.GSX_ERR_INVALID_ARG, _lib.GSX_ERR_NOT_FOUND, _lib.GSX_ERR_UNSUPPORTED
        nan = float("nan")
        out, hit, selected = _lib.PlaneFit(), C.c_uint64(), C.c_uint64()
        planes = F([[0, 0, 1, 0]])

        def fit_desc(**kw):
            d = _lib.PlaneFitDesc()
            L.gsx_plane_fit_desc_default(C.byref(d))
            d.tolerance = 0.01
            for k, val in kw.items():
                if k in ("toward", "reserved"):
                    for i, x in enumerate(val):
                        getattr(d, k)[i] = x
                else:
                    setattr(d, k, val)
            return d

        def sel_desc(**kw):
            d = _lib.PlaneSelectDesc()
            L.gsx_plane_select_desc_default(C.byref(d))
            d.lo, d.hi = -1.0, 1.0
            for k, val in kw.items():
                if k == "normal":
                    for i, x in enumerate(val):
                        d.plane.normal[i] = x
                elif k == "offset":
                    d.plane.offset = val
                elif k == "reserved":
                    for i, x in enumerate(val):
                        d.reserved[i] = x
                else:
                    setattr(d, k, val)
            return d

        fit = lambda d, key=b"src", cand=None, viewer=h, o=out: L.gsx_model_fit_plane(viewer, key, C.byref(d) if d is not None else None, cand, None, None,  # noqa: E731
                                                                                      C.byref(o) if o is not None else None)
        select = lambda d, key=b"src", viewer=h: L.gsx_model_select_plane(viewer, key, C.byref(d) if d is not None else None, C.byref(hit), C.byref(selected))  # noqa: E731
        sb = m.gaussian_buffers.selection_buffer
        sb.upload(X.words(np.arange(200) % 2 == 0))
        before = sb.download().tobytes()
        assert fit(fit_desc()) == _lib.GSX_OK
        for bad in (dict(filter=8), dict(flags=2), dict(sample=3), dict(n_candidates=0), dict(n_candidates=1025), dict(tolerance=-0.5), dict(tolerance=nan),
                    dict(tolerance=INF), dict(min_cos=-0.1), dict(min_cos=1.5), dict(min_cos=nan), dict(refine_iters=9), dict(orient=2),
                    dict(orient=1, toward=(nan, 0, 0)), dict(sample=PR.CALLER), dict(reserved=(1, 0, 0)), dict(reserved=(0, 1, 0)), dict(reserved=(0, 0, 7))):
            assert fit(fit_desc(**bad)) == INV and b"gsx_model_fit_plane" in L.gsx_last_error_string(), bad
        assert fit(None) == INV and fit(fit_desc(), key=None) == INV and fit(fit_desc(), viewer=None) == INV and fit(fit_desc(), o=None) == INV
        assert fit(fit_desc(), key=b"nope") == NF
        assert fit(fit_desc(sample=PR.CALLER, n_candidates=1), cand=planes.ctypes.data) == _lib.GSX_OK
        for bad in (dict(filter=8), dict(selection_op=3), dict(lo=1.0, hi=0.5), dict(lo=nan), dict(hi=nan), dict(min_cos=-0.5), dict(min_cos=2.0), dict(min_cos=nan),
                    dict(normal=(0, 0, 0)), dict(normal=(nan, 0, 1)), dict(normal=(0, INF, 1)), dict(offset=nan), dict(offset=INF), dict(reserved=(1, 0, 0))):
            assert select(sel_desc(**bad)) == INV and b"gsx_model_select_plane" in L.gsx_last_error_string(), bad
        assert select(None) == INV and select(sel_desc(), key=None) == INV and select(sel_desc(), viewer=None) == INV
        assert select(sel_desc(), key=b"nope") == NF
        assert sb.download().tobytes() == before  # a refused call leaves the selection as it was
        assert L.gsx_model_select_plane(h, b"src", C.byref(sel_desc(lo=-INF, hi=INF)), None, None) == _lib.GSX_OK  # (the counts are optional)
        # a model of 0 Gaussians, 0 participants
        v.add_model("empty", 0)
        none = v.models["empty"].fit_plane(0.01)
        assert none.degenerate and (none.count, none.n_valid, none.n_inliers) == (0, 0, 0) and none.winner is None and not none.plane.any()
        assert v.models["empty"].select_plane([0, 0, 1, 0], -1, 1) == (0, 0)
        sb.upload(X.words(np.zeros(200, bool)))
        none = m.fit_plane(0.01, filter=X.SELECTED)
        assert none.degenerate and (none.count, none.n_valid) == (0, 0) and not none.candidates.any() and not none.counts.any()
        # a sharded model; a viewer with a communicator
        _frames(v, ["src"], poses=(5,))
        _load(v, g[:50], "b")
        v.shard_set_limits("b", np.full((FB_H + 15) // 16 * ((FB_W + 15) // 16), 0x40400000, np.uint32))
        _load(other, g[:50], "a")
        other.comm_init_group(CommGroup(1), 0)
        for model, word in ((v.models["b"], "shard"), (other.models["a"], "communicator")):
            for call in (lambda: model.fit_plane(0.01), lambda: model.select_plane([0, 0, 1, 0], -1, 1)):
                with pytest.raises(GsxError, match=word) as err:
                    call()
                assert err.value.status == UNS
