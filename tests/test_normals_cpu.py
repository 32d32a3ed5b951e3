"""CPU tests of the road-plane removal: the float64 restatement of its semantics (tests/_normals_ref.py) against scipy's cKDTree and against
its own stated rules, and the C ABI's new entry points.  The semantics are the project's own statement of Open3D's hybrid search and
covariance normals; Open3D is installed nowhere this could run, so no test here or on the GPU compares with Open3D."""
import os
import re

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from sdflabel_amd import frame as FR
from sdflabel_amd.pipelines import refinement as rtools
from tests import _normals_ref as NR
from tests._util import ROOT

NEW = ("sdfr_lidar_normals_ws_bytes", "sdfr_lidar_normals", "sdfr_depth_map_masked")


def test_restatement_agrees_with_ckdtree_on_neighbour_counts_and_sets():
    from scipy.spatial import cKDTree
    P = NR.street(1)
    ref = NR.normals(P, NR.KITTI_K, *NR.KITTI_WH)
    idx = np.nonzero(ref["in_frustum"])[0]
    assert 0 < len(idx) < len(P)                                                  # some of the scene is outside the frustum
    dist, nn = cKDTree(P[idx]).query(P[idx], k=30, distance_upper_bound=1.0)
    counts = np.isfinite(dist).sum(1)
    # (cKDTree keeps d <= 1; the scene has no pair at exactly 1 m, which the second assertion checks through the sets)
    assert np.array_equal(counts, ref["nn_count"][idx])
    assert (ref["nn_count"][~ref["in_frustum"]] == 0).all()
    for a, i in enumerate(idx):
        assert set(idx[nn[a, :counts[a]]].tolist()) == set(ref["nn_idx"][i, :counts[a]].tolist())
    assert (counts < 3).sum() > 100 and (counts == 30).sum() > 200                # both regimes are there
    assert not ref["cut_tie"].any() and NR.excluded(ref).sum() <= 0.02 * len(P)


def test_restatement_is_bit_invariant_under_a_permutation():
    P = NR.street(2)
    ref = NR.normals(P, NR.KITTI_K, *NR.KITTI_WH)
    assert not ref["cut_tie"].any()                                               # without ties the index plays no part
    perm = np.random.default_rng(0).permutation(len(P))
    got = NR.normals(P[perm], NR.KITTI_K, *NR.KITTI_WH)
    assert got["normals"].tobytes() == ref["normals"][perm].tobytes()
    assert np.array_equal(got["nn_count"], ref["nn_count"][perm]) and np.array_equal(got["keep"], ref["keep"][perm])
    inv = np.argsort(perm)                                                        # old index -> new index
    mapped = np.where(ref["nn_idx"][perm] >= 0, inv[np.maximum(ref["nn_idx"][perm], 0)], -1)
    assert np.array_equal(got["nn_idx"], mapped)


def test_fewer_than_three_neighbours_and_degenerate_clouds_give_the_default_normal():
    P = NR.f32([[0, 0, 10], [0.1, 0, 10], [5, 0, 10], [5, 0.1, 10.2], [5.1, 0.3, 10], [20, 0, 10]])
    ref = NR.normals(P)
    assert ref["nn_count"].tolist() == [2, 2, 3, 3, 3, 1]
    assert np.array_equal(ref["normals"][[0, 1, 5]], np.tile([0.0, 0.0, 1.0], (3, 1)))
    n = ref["normals"][2:5]
    assert np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-15) and (np.einsum("ij,ij->i", n, P[2:5]) <= 0).all()
    same = NR.normals(np.tile(NR.f32([[1.5, 0.25, 7.0]]), (30, 1)))                   # a zero covariance
    assert (same["nn_count"] == 30).all() and np.array_equal(same["normals"], np.tile([0.0, 0.0, 1.0], (30, 1)))
    assert np.array_equal(same["nn_idx"][7], np.arange(30))                       # all at distance 0: by index


def test_the_radius_is_a_strict_bound_on_a_half_metre_lattice():
    g = np.arange(5) * 0.5
    P = NR.f32(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + [0.0, 0.0, 8.0])
    ref = NR.normals(P, radius=1.0, max_nn=64)
    centre = int(np.nonzero((P == [1.0, 1.0, 9.0]).all(1))[0][0])
    # within 1 m strictly: d2 in {0, .25, .5, .75}: 1 + 6 + 12 + 8; the six lattice points at exactly 1 m are out
    assert ref["nn_count"][centre] == 27
    d2 = ((P[ref["nn_idx"][centre, :27]] - P[centre]) ** 2).sum(1)
    assert d2.max() == 0.75 and (np.diff(d2) >= 0).all()
    half = NR.normals(P, radius=0.5, max_nn=64)
    assert (half["nn_count"] == 1).all()                                          # the neighbours at exactly 0.5 m are out as well


def test_new_entry_points_are_exported_declared_and_bound():
    """fails before the feature: the ABI has no lidar-normal entry points"""
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    h = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint(?:64_t)?\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(h, name)
    assert int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == h.sdfr_version() >= 408
    for fn in ("lidar_normals", "remove_road", "kitti_frame"):
        assert callable(getattr(FR, fn))
    assert callable(rtools.get_kitti_frame)
    import inspect
    from sdflabel_amd.pipelines.frame import refine_sample
    assert inspect.signature(refine_sample).parameters["remove_road"].default is False
    # the workspace grows with N and is refused beyond the limit
    assert 0 < h.sdfr_lidar_normals_ws_bytes(0) < h.sdfr_lidar_normals_ws_bytes(1000) < h.sdfr_lidar_normals_ws_bytes(120000)
    assert h.sdfr_lidar_normals_ws_bytes(-1) == -1
    # read from the library as it was before the grid's arrays were carved by hash_grid.h: callers' allocations must not change
    before = {0: 528, 1: 608, 31: 1920, 32: 1936, 33: 2528, 1000: 60400, 120000: 7377168}
    for n, want in before.items():
        assert h.sdfr_lidar_normals_ws_bytes(n) == want, n
    # argument validation happens before any HIP call
    assert h.sdfr_lidar_normals(None, 1, 10, None, 1.0, 30, None, None, None, None, None, 0, None) == -1 and b"NULL" in h.sdfr_last_error()
    assert h.sdfr_lidar_normals(None, 1, 10, None, 1.0, 65, None, None, None, None, None, 0, None) == -1 and b"max_nn" in h.sdfr_last_error()
    assert h.sdfr_lidar_normals(None, 1, 10, None, 0.0, 30, None, None, None, None, None, 0, None) == -1 and b"radius" in h.sdfr_last_error()
    assert h.sdfr_lidar_normals(None, 1, -1, None, 1.0, 30, None, None, None, None, None, 0, None) == -1
    assert h.sdfr_lidar_normals(None, 1, 0, None, 1.0, 30, None, None, None, None, None, 0, None) == 0
    assert h.sdfr_depth_map_masked(None, 1, 10, None, None, None, 8, 8, None, None, None, None) == -1 and b"NULL" in h.sdfr_last_error()


def test_grid_rules_on_the_host_find_the_radius_graphs_components(tmp_path):
    """csrc/hash_grid.h is one header for the normals and the clusters, and tests/cluster_host is its host build.  Run with eps = the
    normals' radius and the frustum as the mask, the harness walks the normals' grid (cell width from the radius, clamp, 27 cells, bucket
    collisions) over the normals' points; its components must be those of the radius graph, which scipy finds without any grid."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    from tests import _cluster_ref as CR
    from tests._util import build_host_program
    from tests.test_cluster_cpu import _near_threshold, _run_host
    radius = 1.0
    P = np.ascontiguousarray(NR.street(1)[:900], np.float32)
    inside = NR.in_frustum(P, NR.KITTI_K, *NR.KITTI_WH)
    idx = np.nonzero(inside)[0]
    assert 100 < len(idx) < len(P) and not _near_threshold(P, inside, radius)     # scipy keeps d <= radius, the rule is strict: no pair is at it
    case = {"points": P, "mask": inside.astype(np.uint8), "kw": dict(eps=radius, min_points=1, max_points=None, max_clusters=1024)}
    exe = build_host_program(tmp_path, "cluster_host/cluster_host.cpp", "cluster_host")
    label, _, _, counts, _ = _run_host(exe, tmp_path, case, CR.directions(1), 0)
    pr = cKDTree(P[idx].astype(np.float64)).query_pairs(radius, output_type="ndarray")
    ncomp, lab = connected_components(coo_matrix((np.ones(len(pr)), (pr[:, 0], pr[:, 1])), shape=(len(idx), len(idx))), directed=False)
    assert 1 < ncomp < len(idx) and counts.tolist() == [len(idx), ncomp, ncomp, 0]
    assert (label[~inside] == -1).all() and (label[idx] >= 0).all()
    # the same partition: one scipy label per component number and one component number per scipy label
    assert len(set(zip(lab.tolist(), label[idx].tolist()))) == ncomp


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)              # host inputs and no GPU: a loud refusal, never a host computation
    P = torch.from_numpy(NR.street(3)[:50])
    K, (w, h) = NR.KITTI_K, NR.KITTI_WH
    image = torch.zeros((h, w, 3))
    with pytest.raises(_lib.SdfrError):
        FR.lidar_normals(P)
    with pytest.raises(_lib.SdfrError):
        FR.lidar_normals(P, K, w, h)
    with pytest.raises(_lib.SdfrError):
        FR.remove_road(P, K, w, h)
    with pytest.raises(_lib.SdfrError):
        FR.kitti_frame(image, P, K)
    with pytest.raises(_lib.SdfrError):
        rtools.get_kitti_frame({"image": image.numpy(), "lidar": P.numpy(), "orig_cam": K})
