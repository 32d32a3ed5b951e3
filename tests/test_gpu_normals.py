"""The road-plane removal on the GPU (csrc/normals.hip, the masked depth map of csrc/ingest.hip, sdflabel_amd/frame.py lidar_normals /
remove_road / kitti_frame, pipelines/refinement.py get_kitti_frame, pipelines/frame.py refine_sample(remove_road=True)) against the float64
restatement of its semantics in tests/_normals_ref.py, which tests/test_normals_cpu.py pins to scipy's cKDTree and to the stated rules.
The semantics are the project's own statement of Open3D's hybrid search and covariance normals: NOTHING here compares with Open3D.

Neighbour counts and indices are compared for equality: the scenes hold float32 values, so d2 has the same bits on both sides.
Normals: the covariance is a centred sum of at most 30 terms, relative error about 4e-15 on either side; by Davis-Kahan the eigenvector
turns by that over gap = (l1 - l0) / l2, so the bound is 1e-13 / gap (a margin of about 25 on that estimate; the largest error x gap observed on an MI355X is 4.7e-16,
profiles/normals_notes.md).  The road flag is compared on every point but
those the restatement itself marks undecidable (gap < 1e-3, |n_y| within 1e-9 of the cut, a cut tie), which may be at most 2 % of a scene.
Figures are printed before they are asserted."""
import warnings

import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import frame as FR
from sdflabel_amd.pipelines import refinement as rtools
from tests import _normals_ref as NR
from tests._util import ASSET

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, (W, H) = NR.KITTI_K, NR.KITTI_WH
SEEDS = (1, 2, 3)


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message).lower() for x in w), out


@pytest.fixture(scope="module")
def streets():
    """seed -> (points, restatement); computed once, never modified"""
    out = {}
    for s in SEEDS:
        P = NR.street(s)
        out[s] = (P, NR.normals(P, K, W, H))
    return out


def run(P, *a, **k):
    n, info = FR.lidar_normals(P, *a, return_info=True, **k)
    return n.cpu().numpy(), info["nn_count"].cpu().numpy(), info["nn_idx"].cpu().numpy(), info["in_frustum"].cpu().numpy()


def normal_error(got, ref, P):
    """per point |got - ref|, up to the sign where n . p is too close to 0 for the sign rule to be decidable"""
    e = np.linalg.norm(got - ref["normals"], axis=1)
    flat = np.abs(np.einsum("ij,ij->i", ref["normals"], P)) < 1e-9
    return np.where(flat, np.minimum(e, np.linalg.norm(got + ref["normals"], axis=1)), e)


def check_against(P, ref, got, label):
    n, cnt, idx, inside = got
    tol = np.minimum(1e-13 / np.maximum(ref["gap"], 1e-300), 2.5)
    err = normal_error(n, ref, P)
    fin = np.isfinite(ref["gap"])
    worst = float((err[fin] * ref["gap"][fin]).max()) if fin.any() else 0.0
    print("%s: %d points, %d in the frustum, %d with < 3 neighbours, %d at the cap; %d counts, %d index rows differ; largest error x gap %.3g "
          "(bound 1e-13); largest error %.3g" % (label, len(P), int(inside.sum()), int((cnt[inside] < 3).sum()), int((cnt == idx.shape[1]).sum()),
                                                 int((cnt != ref["nn_count"]).sum()), int((idx != ref["nn_idx"]).any(1).sum()), worst, float(err.max())))
    assert np.array_equal(inside, ref["in_frustum"])
    assert np.array_equal(cnt, ref["nn_count"]) and np.array_equal(idx, ref["nn_idx"])
    assert (err <= tol).all()
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-14, rtol=0)
    return worst


@pytest.mark.parametrize("seed", SEEDS)
def test_street_scene_equals_the_restatement(streets, seed):
    P, ref = streets[seed]
    worst = check_against(P, ref, run(P, K, W, H), "street %d" % seed)
    keep, info = FR.remove_road(P, K, W, H, return_info=True)
    keep = keep.cpu().numpy()
    ex = NR.excluded(ref)
    road = info["in_frustum"].cpu().numpy() & ~keep
    print("street %d: %d road points (restatement %d), %d excluded (%.2f %%), %d flags differ outside them; error x gap %.3g" %
          (seed, int(road.sum()), int(ref["road"].sum()), int(ex.sum()), 100.0 * ex.sum() / len(P), int((road != ref["road"])[~ex].sum()), worst))
    assert keep.dtype == bool and ex.sum() <= 0.02 * len(P)
    assert np.array_equal(road[~ex], ref["road"][~ex]) and np.array_equal(keep[~ex], ref["keep"][~ex])
    assert 0.3 * len(P) < road.sum() < 0.7 * len(P)                               # the ground is found, the cars and the rest stay
    assert torch.equal(info["normals"], FR.lidar_normals(P, K, W, H))


def test_dense_blob_returns_the_exact_thirty_nearest_of_three_thousand():
    P = NR.blob()
    ref = NR.normals(P)
    got = run(P)
    check_against(P, ref, got, "blob")
    assert (got[1] == 30).all() and got[3].all()


def test_shuffled_lattice_cuts_ties_by_index():
    P = NR.lattice()
    ref = NR.normals(P)
    n, cnt, idx, _ = run(P)
    print("lattice: %d points, %d cut on an exact tie, %d index rows differ" % (len(P), int(ref["cut_tie"].sum()), int((idx != ref["nn_idx"]).any(1).sum())))
    assert ref["cut_tie"].sum() > 300
    assert np.array_equal(cnt, ref["nn_count"]) and np.array_equal(idx, ref["nn_idx"])
    assert np.isfinite(n).all() and np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-14, rtol=0)      # degenerate covariances: not compared


def test_edges():
    default = np.array([0.0, 0.0, 1.0])
    for npts in (0, 1, 2):
        P = NR.f32(np.array([[0.0, 0.5, 9.0], [0.1, 0.5, 9.0]])[:npts].reshape(-1, 3))
        n, cnt, idx, inside = run(P, K, W, H)
        assert n.shape == (npts, 3) and idx.shape == (npts, 30) and cnt.tolist() == [npts] * npts and inside.all()
        assert np.array_equal(n, np.tile(default, (npts, 1)))
        keep = FR.remove_road(P, K, W, H)
        assert keep.shape == (npts,) and keep.all()
    behind = NR.f32(np.random.default_rng(4).normal(0, 1, (200, 3)) - [0, 0, 20.0])    # all outside the frustum
    n, cnt, idx, inside = run(behind, K, W, H)
    assert not inside.any() and not cnt.any() and (idx == -1).all() and np.array_equal(n, np.tile(default, (200, 1)))
    assert not FR.remove_road(behind, K, W, H).any()
    same = np.tile(NR.f32([[1.5, 0.25, 7.0]]), (30, 1))                             # a zero covariance
    n, cnt, idx, _ = run(same)
    assert (cnt == 30).all() and np.array_equal(idx, np.tile(np.arange(30), (30, 1))) and np.array_equal(n, np.tile(default, (30, 1)))
    line = NR.f32([[0.0, 0.0, 5.0], [0.125, 0.125, 5.25], [0.25, 0.25, 5.5]])        # collinear, within 1 m: a null space of dimension 2
    n, cnt, _, _ = run(line)
    d = (line[2] - line[0]) / np.linalg.norm(line[2] - line[0])
    print("collinear: normals %s, |n . direction| %s" % (n.tolist(), np.abs(n @ d).tolist()))
    assert cnt.tolist() == [3, 3, 3] and np.isfinite(n).all() and np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-14, rtol=0)
    assert (np.abs(n @ d) < 1e-7).all()
    P = NR.street(1)[:900]
    for kw in ({"max_nn": 3}, {"max_nn": 64}, {"radius": 0.5}, {"radius": 0.5, "max_nn": 5}):
        check_against(P, NR.normals(P, K, W, H, **kw), run(P, K, W, H, **kw), "street 1, first 900, %s" % kw)
    with pytest.raises(ValueError):
        FR.lidar_normals(P, max_nn=65)
    with pytest.raises(ValueError):
        FR.lidar_normals(P, radius=0.0)


def test_a_neighbour_outside_the_frustum_does_not_count():
    Ks, w, h = NR.small_camera()
    pl = NR.R.frustum_planes(Ks, 0, 0, w, h).astype(np.float64)
    rng = np.random.default_rng(12)
    z = rng.uniform(6.0, 12.0, 600)
    edge = (w - 1 - Ks[0, 2]) / Ks[0, 0]                                             # the right plane: x = edge z
    P = NR.f32(np.stack([edge * z + rng.uniform(-0.8, 0.8, 600), rng.uniform(-0.3, 0.3, 600), z], 1))
    ref = NR.normals(P, Ks, w, h)
    everyone = NR.normals(P)
    inside = ref["in_frustum"]
    assert 150 < inside.sum() < 450 and (np.abs(pl @ P.T) > 1e-9).all()              # both sides of the plane, none on it
    assert (everyone["nn_idx"][inside] != ref["nn_idx"][inside]).any(1).sum() > 100  # the cut changes the neighbours: the test can tell
    check_against(P, ref, run(P, Ks, w, h), "straddling the right plane")
    check_against(P, everyone, run(P), "the same cloud without a frustum")


def test_two_runs_and_a_permutation_give_the_same_bits(streets):
    P, ref = streets[1]
    a, b = run(P, K, W, H), run(torch.from_numpy(P).to(DEV), torch.from_numpy(K), W, H)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    perm = np.random.default_rng(5).permutation(len(P))
    inv = np.argsort(perm)
    n, cnt, idx, inside = run(P[perm], K, W, H)
    assert not ref["cut_tie"].any()
    assert n.tobytes() == a[0][perm].tobytes() and np.array_equal(cnt, a[1][perm]) and np.array_equal(inside, a[3][perm])
    assert np.array_equal(idx, np.where(a[2][perm] >= 0, inv[np.maximum(a[2][perm], 0)], -1))
    k1, k2 = FR.remove_road(P, K, W, H), FR.remove_road(P[perm], K, W, H)
    assert torch.equal(k1[torch.from_numpy(perm).to(DEV)], k2)


def test_float32_input_gives_the_bits_of_the_widened_input(streets):
    P, _ = streets[2]
    a, b = run(P, K, W, H), run(P.astype(np.float32), K, W, H)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert torch.equal(FR.remove_road(P, K, W, H), FR.remove_road(torch.from_numpy(P.astype(np.float32)).to(DEV), K, W, H))


# ---- the depth map, the frame and the sample --------------------------------------------------------------------------------------------

def _decided(P, Ks, w, h, keep):
    """the restatement's keep, with the points it marks undecidable taken from the device's answer"""
    ref = NR.normals(P, Ks, w, h)
    ex = NR.excluded(ref)
    assert ex.sum() <= 0.02 * len(P)
    return np.where(ex, keep, ref["keep"]), ref


def test_kitti_frame_equals_the_depth_map_of_the_kept_points(streets):
    Ks, w, h = NR.small_camera()
    P = streets[3][0]
    rng = np.random.default_rng(6)
    image = rng.random((h, w, 3)).astype(np.float32)
    syncs, (depth, pts, clrs, info) = count_syncs(lambda: FR.kitti_frame(image, P, Ks, return_info=True))
    keep = info["keep"].cpu().numpy()
    keep_ref, ref = _decided(P, Ks, w, h, keep)
    want = FR.depth_map(P[keep_ref], Ks, w, h)
    plain = FR.depth_map(P, Ks, w, h)
    print("kitti_frame at %d x %d: %d points, %d kept (restatement %d), %d pixels set (%d with the road), %d depth values differ, %d synchronisations"
          % (w, h, len(P), int(keep.sum()), int(keep_ref.sum()), int((depth != 0).sum()), int((plain != 0).sum()), int((depth != want).sum()), syncs))
    assert np.array_equal(keep, keep_ref) and syncs == 0
    assert depth.is_cuda and depth.dtype == torch.float32 and depth.shape == (h, w) and torch.equal(depth, want)
    assert (plain != 0).sum() > (depth != 0).sum() > 20                             # the road is gone, the rest is there
    assert info["counts"].tolist() == [int(keep.sum()), 0]
    assert keep.sum() > 1.3 * int((depth != 0).sum())                              # several points per pixel: the overwrite order matters
    # the winner indexes the whole cloud
    win = info["winner"].cpu().numpy()
    assert keep[win[win >= 0]].all() and np.array_equal(P[win[win >= 0], 2].astype(np.float32), depth.cpu().numpy()[win >= 0])
    # the scene points are those of reproject on that depth map
    (rp, rc), = FR.reproject_many([image], [want], [Ks])
    n = int(info["count"])
    assert n == int((depth != 0).sum()) and torch.equal(pts[:n], rp) and torch.equal(clrs[:n], rc)
    # the drop-in
    sample = {"image": image, "lidar": P, "orig_cam": Ks}
    syncs2, (d2, pcd) = count_syncs(lambda: rtools.get_kitti_frame(sample))
    print("get_kitti_frame: %d synchronisations before the cloud is converted" % syncs2)
    assert syncs2 == 0 and torch.equal(d2, depth)
    gp, gc = np.asarray(pcd.points), np.asarray(pcd.colors)
    assert gp.dtype == np.float64 and gp.shape == (n, 3) and np.array_equal(gp, rp.cpu().numpy()) and np.array_equal(gc, rc.cpu().numpy())
    d32, _, _ = FR.kitti_frame(torch.from_numpy(image).to(DEV), torch.from_numpy(P.astype(np.float32)).to(DEV), Ks)
    assert torch.equal(d32, depth)


def test_refine_sample_removes_the_road_like_a_pre_filtered_cloud():
    from sdflabel_amd.fixtures import stand_in_css, synthetic_sample
    from sdflabel_amd.pipelines import optimizer as OP
    from sdflabel_amd.pipelines.frame import refine_sample
    dec32 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)
    dec16 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)
    smp, cars = synthetic_sample(dec32, 40, 32, DEV)
    Hs, Ws = smp["image"].shape[:2]
    Ks = smp["orig_cam"]
    # a road under the cars: a grid of about 2 500 points at the cars' lowest point
    rng = np.random.default_rng(9)
    x0, x1, z0, z1 = cars[:, 0].min() - 0.5, cars[:, 0].max() + 0.5, cars[:, 2].min() - 0.5, cars[:, 2].max() + 0.5
    step = max(0.15, float(np.sqrt((x1 - x0) * (z1 - z0) / 2500.0)))
    gx, gz = np.meshgrid(np.arange(x0, x1, step), np.arange(z0, z1, step))
    road = np.stack([gx.ravel(), np.full(gx.size, cars[:, 1].max() + 0.05) + rng.normal(0, 0.003, gx.size), gz.ravel()], 1)
    lidar = NR.f32(np.concatenate([cars, road]))
    keep, info = FR.remove_road(lidar, Ks, Ws, Hs, return_info=True)
    keep = keep.cpu().numpy()
    keep_ref, ref = _decided(lidar, Ks, Ws, Hs, keep)
    inside = ref["in_frustum"]
    road_in = inside[len(cars):]
    print("sample %d x %d: %d car points and %d road points %.2f m apart, %d / %d of them in the frustum, %d / %d kept (restatement %d / %d), "
          "%d undecidable" % (Ws, Hs, len(cars), len(road), step, int(inside[:len(cars)].sum()), int(road_in.sum()), int(keep[:len(cars)].sum()),
                              int(keep[len(cars):].sum()), int(keep_ref[:len(cars)].sum()), int(keep_ref[len(cars):].sum()), int(NR.excluded(ref).sum())))
    assert np.array_equal(keep, keep_ref)
    assert step < 0.45 and road_in.sum() > 50 and keep[len(cars):][road_in].mean() < 0.2 and keep[:len(cars)].sum() > 0.3 * len(cars)
    net = stand_in_css().to(DEV)
    grid = sdflabel_amd.Grid3D(40, DEV)
    W8, iters = {"2d": 0.3, "3d": 0.5}, 10
    OP.clear_refiner_cache()
    est, kept, _, st = refine_sample(smp, net, dec16, grid, iters, W8, lidar=lidar, remove_road=True, seed=7, return_stages=True)
    est2, kept2, _, st2 = refine_sample(smp, net, dec16, grid, iters, W8, lidar=lidar[keep_ref], seed=7, return_stages=True)
    plain = FR.depth_map(lidar, Ks, Ws, Hs)
    print("refine_sample: %d kept; %d pixels of the depth map set with the road removed, %d with it" %
          (len(kept), int((st["depth"] != 0).sum()), int((plain != 0).sum())))
    assert torch.equal(st["depth"], st2["depth"]) and not torch.equal(st["depth"], plain)
    assert kept == kept2 and len(kept) >= 1 and est["name"] == est2["name"]
    for k in FR.NECESSARY_KEYS:
        assert est[k].dtype == est2[k].dtype and est[k].tobytes() == est2[k].tobytes(), k
    s_road = count_syncs(lambda: refine_sample(smp, net, dec16, grid, iters, W8, lidar=lidar, remove_road=True, seed=7))[0]
    s_pre = count_syncs(lambda: refine_sample(smp, net, dec16, grid, iters, W8, lidar=lidar[keep_ref], seed=7))[0]
    print("host synchronisations per call: %d with remove_road, %d with the pre-filtered cloud" % (s_road, s_pre))
    assert s_road == s_pre                                                        # the removal adds none
    with pytest.raises(ValueError):
        refine_sample(smp, net, dec16, grid, iters, W8, remove_road=True)
