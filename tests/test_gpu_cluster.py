"""Lidar clusters and rough boxes on the GPU (csrc/cluster.hip, sdflabel_amd/cluster.py, pipelines/scan.py) against the numpy restatement
tests/_cluster_ref.py, which tests/test_cluster_cpu.py pins to scipy and to the host build of csrc/cluster_cells.h.  There is no sum of
floats anywhere in this stage, so everything is compared bit for bit, between guard words -- including the member slots and rectangle rows
that must stay unwritten.  The planted scene is built and checked on the CPU (the restatement finds exactly the planted objects); here the
device only has to equal the restatement.  How good the fit from these starts is, is reported and not asserted."""
import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import cluster as C
from sdflabel_amd import frame as FR
from sdflabel_amd.align import align_many
from sdflabel_amd.pipelines import scan
from tests import _cluster_ref as CR
from tests import _normals_ref as NR
from tests.test_gpu_encode import DEV, Guarded, count_syncs, gpu_decoder, same_bits

pytestmark = pytest.mark.gpu
ALL = [("cluster", n) for n in CR.cluster_cases()] + [("box", n) for n in CR.box_cases()]


def _case(kind, name):
    if kind == "cluster":
        case, ref = CR.cluster_cases()[name], CR.cluster_refs()[name]
        dirs = CR.directions(7)
        return case, dirs, ref, CR.rectangles(case["points"], ref, dirs)
    case = CR.box_cases()[name]
    return (case, case["dirs"]) + CR.box_refs()[name]


def run_guarded(points, mask, kw, dirs):
    """both kernels into buffers between guard words: (label, members, off, counts, rect as numpy, all guards intact)"""
    N, cap = len(points), kw["max_clusters"]
    bufs = [Guarded(N, torch.int32), Guarded(N, torch.int32), Guarded(cap + 1, torch.int32), Guarded(4, torch.int32)]
    rect = Guarded(cap * 8, torch.float64)
    pts = torch.from_numpy(np.array(points)).to(DEV)
    m = None if mask is None else torch.from_numpy(np.array(mask)).to(DEV)
    cl = C.clusters(pts, m, _out=tuple(b.t for b in bufs), **kw)
    C.boxes(None, cl, dirs=dirs, _out=rect.t.view(cap, 8))
    torch.cuda.synchronize()
    return [b.numpy() for b in bufs] + [rect.numpy((cap, 8))], all(b.intact() for b in bufs + [rect]), (bufs[1].sent, rect.sent)


def check(got, ref, want_rect, sent, what):
    label, members, off, counts, rect = got
    total, kept = int(ref["off"][ref["kept"]]), ref["kept"]
    same_bits(counts, ref["counts"], what + " counts"); same_bits(off, ref["off"], what + " off"); same_bits(label, ref["label"], what + " label")
    same_bits(members[:total], ref["members"], what + " members")
    assert (members[total:] == sent[0]).all() and (rect[kept:] == sent[1]).all(), what       # what must stay unwritten
    same_bits(rect[:kept], want_rect, what + " rect")


@pytest.mark.parametrize("kind,name", ALL, ids=["%s-%s" % a for a in ALL])
def test_kernels_equal_the_restatement_bit_for_bit_between_guard_words(kind, name):
    case, dirs, ref, want_rect = _case(kind, name)
    got, intact, sent = run_guarded(case["points"], case["mask"], case["kw"], dirs)
    print("%s: %d points, counts %s, kept %d, K %d" % (name, len(case["points"]), got[3].tolist(), ref["kept"], len(dirs)))
    assert intact
    check(got, ref, want_rect, sent, name)


@pytest.mark.parametrize("name", ("chain", "n2049", "far_cells", "cell_boundaries"))
def test_same_bits_twice_and_components_survive_a_permutation(name):
    case, ref = CR.cluster_cases()[name], CR.cluster_refs()[name]
    dirs = CR.directions(33)
    a, ok_a, _ = run_guarded(case["points"], case["mask"], case["kw"], dirs)
    b, ok_b, _ = run_guarded(case["points"], case["mask"], case["kw"], dirs)
    assert ok_a and ok_b
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    N = len(case["points"])
    perm = np.random.default_rng(5).permutation(N)
    p, ok_p, _ = run_guarded(case["points"][perm], None if case["mask"] is None else case["mask"][perm], case["kw"], dirs)
    assert ok_p and p[3].tolist() == a[3].tolist()
    kept = ref["kept"]
    sets = lambda g, idx: sorted(tuple(sorted(idx[g[1][g[2][c]:g[2][c + 1]]].tolist())) for c in range(kept))       # noqa: E731
    assert sets(p, perm) == sets(a, np.arange(N))                               # the same components, as sets of the original indices
    firsts = [int(p[1][p[2][c]]) for c in range(kept)]
    assert firsts == sorted(firsts)                                             # numbered by the NEW smallest member index
    for c in range(kept):
        assert (np.diff(p[1][p[2][c]:p[2][c + 1]]) > 0).all()
    # a rectangle is a function of the set of points: the permuted run's rectangles are the first run's, found by their members
    mine = {frozenset(a[1][a[2][c]:a[2][c + 1]].tolist()): a[4][c].tobytes() for c in range(kept)}
    for c in range(kept):
        assert p[4][c].tobytes() == mine[frozenset(perm[p[1][p[2][c]:p[2][c + 1]]].tolist())], (name, c)


def test_no_synchronisation_in_clusters_and_boxes_and_one_in_proposals():
    sc, s = CR.planted_scene(), CR.SCENE
    pts, mask = torch.from_numpy(np.array(sc["points"])).to(DEV), torch.from_numpy(np.array(sc["mask"])).to(DEV)
    kw = dict(eps=s["eps"], min_points=s["min_points"], max_clusters=64)
    cl = C.clusters(pts, mask, **kw)                                            # the library is loaded
    C.boxes(None, cl, s["n_angles"])
    syncs, cl = count_syncs(lambda: C.clusters(pts, mask, **kw))
    assert syncs == 0, syncs
    syncs, bx = count_syncs(lambda: C.boxes(None, cl, s["n_angles"]))
    assert syncs == 0, syncs
    assert cl.label.is_cuda and cl.members.is_cuda and cl.offsets.is_cuda and cl.counts.is_cuda and bx.rect.is_cuda
    lat = torch.from_numpy(np.array(sc["z_true"])).to(DEV)
    syncs, props = count_syncs(lambda: C.proposals(pts, mask, n_angles=s["n_angles"], scale=s["scale"], latent=lat, gates=s["gates"], **kw))
    assert syncs == 1, syncs
    assert len(props) == 3


def _yaw_error(y, truth):
    return abs((y - truth + np.pi / 2) % np.pi - np.pi / 2)


def test_proposals_on_the_planted_scene_are_the_restatements():
    sc, s = CR.planted_scene(), CR.SCENE
    P = sc["points"]
    kw = dict(eps=s["eps"], min_points=s["min_points"], max_clusters=64)
    ref = CR.clusters(P, sc["mask"], **kw)
    dirs = CR.directions(s["n_angles"])
    rect = CR.rectangles(P, ref, dirs)
    props = C.proposals(torch.from_numpy(np.array(P)).to(DEV), torch.from_numpy(np.array(sc["mask"])).to(DEV), n_angles=s["n_angles"], scale=s["scale"],
                        latent=sc["z_true"], gates=s["gates"], **kw)
    same_bits(props.counts, ref["counts"]); same_bits(props.offsets, ref["off"]); same_bits(props.rect, rect)
    same_bits(props.clusters.label.cpu().numpy(), ref["label"])
    yaw, trans, dims = C.starts_from_rect(rect, dirs, s["scale"])
    assert len(props) == 3 and [i["cluster"] for i in props.info] == [c for c in range(ref["kept"]) if dims[c, 0] <= s["gates"]["length"][1]]
    seen = set()
    for a, (prm, cloud, info) in enumerate(props):
        c = info["cluster"]
        m = ref["members"][ref["off"][c]:ref["off"][c + 1]]
        same_bits(cloud.cpu().numpy(), P[m], "the cloud is the cluster's points in input order")
        same_bits(info["rect"], rect[c])
        who = int(np.unique(sc["owner"][m])[0])
        seen.add(who)
        y_true, centre = sc["truth"][who]
        assert prm["yaw"].dtype == torch.float32 and tuple(prm["trans"].shape) == (3,) and tuple(prm["scale"].shape) == (1,) and tuple(prm["latent"].shape) == (3,)
        assert float(prm["yaw"]) == np.float32(yaw[c]) and float(props.flipped[a]["yaw"]) == np.float32(yaw[c] + np.pi)
        same_bits(prm["trans"].cpu().numpy(), trans[c].astype(np.float32)); same_bits(props.flipped[a]["trans"].cpu().numpy(), trans[c].astype(np.float32))
        print("object %d: cluster %d, %d points, dims %s; start yaw error (mod pi) %.3f rad, centre error %s m" %
              (who, c, info["n"], np.round(info["dims"], 2), _yaw_error(yaw[c], y_true), np.round(info["centre"] - centre, 2)))
    assert seen == {0, 1, 2}


def _chain(dec, grid, pts, mask, K, w, h, p_WC, lat, ckw, akw):
    """label_scan's five calls written out by hand (without the road removal when a mask is given)"""
    keep = FR.remove_road(pts, K, w, h) if mask is None else mask
    props = C.proposals(pts, keep, latent=lat, **ckw)
    A = len(props)
    fits = align_many(dec, props.params + props.flipped, props.clouds + props.clouds, **akw)
    loss = fits.loss.cpu().numpy()
    second = np.array([(loss[A + a] < loss[a]) or (np.isnan(loss[a]) and not np.isnan(loss[A + a])) for a in range(A)], bool)
    theta, lats = fits.theta.cpu().numpy(), fits.latents.cpu().numpy()
    params = [{"yaw": theta[a + A * second[a], 0:1], "trans": theta[a + A * second[a], 1:4], "scale": theta[a + A * second[a], 4:5],
               "latent": lats[a + A * second[a]]} for a in range(A)]
    off = torch.tensor([int(props.offsets[i["cluster"]]) for i in props.info], dtype=torch.int64, device=DEV)
    cnt = torch.tensor([i["n"] for i in props.info], dtype=torch.int32, device=DEV)
    Kd = torch.from_numpy(np.tile(np.asarray(K, np.float32).reshape(1, 9), (A, 1))).to(DEV)
    ext, _ = FR.point_extents(props.gathered, off, cnt, int(cnt.max()), A, K=Kd)
    uv = ext[:, 6:10].cpu().numpy()
    bboxes = [np.array([np.clip(r[0], 0, w), np.clip(r[2], 0, h), np.clip(r[1], 0, w), np.clip(r[3], 0, h)], np.float32) for r in uv]
    labels = FR.labels_many(dec, grid, params, p_WC, bboxes)
    return FR.frame_dict(labels), props, fits, second, bboxes


@pytest.mark.parametrize("road", (False, True), ids=("given_mask", "remove_road"))
def test_label_scan_equals_the_hand_written_chain_of_its_calls(road):
    sc, s = CR.planted_scene(), CR.SCENE
    K, (w, h) = NR.KITTI_K, NR.KITTI_WH
    dec, grid = gpu_decoder("asset"), sdflabel_amd.Grid3D(40, DEV)
    p_WC = np.eye(4)
    p_WC[:3, 3] = [0.1, -0.2, 0.3]
    P = sc["points"] if road else sc["points"][sc["mask"] != 0]                  # (with a mask given: the road-free points, every one taking part)
    pts = torch.from_numpy(np.array(P)).to(DEV)
    lat = torch.from_numpy(np.array(sc["z_true"])).to(DEV)
    ckw = dict(eps=s["eps"], min_points=s["min_points"], max_clusters=64, n_angles=s["n_angles"], scale=s["scale"], gates=s["gates"])
    akw = dict(iters=60, rows_per_iter=512, lr_step=40, seed=3)
    want, props, fits, second, bboxes = _chain(dec, grid, pts, None if road else torch.ones(len(P), dtype=torch.uint8, device=DEV), K, w, h, p_WC, lat, ckw, akw)
    syncs, (est, st) = count_syncs(lambda: scan.label_scan(dec, grid, pts, K, w, h, p_WC, lat, remove_road=road, cluster_kw=ckw, align_kw=akw))
    A = len(st["proposals"])
    print("label_scan (%s): %d proposals, %d synchronisations, second hypothesis chosen %s, losses %s" %
          ("remove_road" if road else "given mask", A, syncs, st["second"].tolist(), None if st["fits"] is None else st["fits"].loss.cpu().numpy()))
    assert syncs == (2 + (A + 15) // 16 if A else 1), syncs                       # as label_scan's docstring states
    assert A == len(props) and set(est) == set(want)
    for k in want:
        assert (list(est[k]) == list(want[k])) if k == "name" else (est[k].dtype == want[k].dtype and est[k].tobytes() == want[k].tobytes()), k
    assert torch.equal(st["fits"].theta, fits.theta) and torch.equal(st["fits"].latents, fits.latents) and torch.equal(st["fits"].loss, fits.loss)
    assert st["second"].tolist() == second.tolist() and all(a.tobytes() == b.tobytes() for a, b in zip(st["bboxes"], bboxes))
    if road:
        return
    assert A == 3 and len(est["name"]) == 3 and st["proposals"].counts[3] == 0
    loss, flags = fits.loss.cpu().numpy(), fits.flags.cpu().numpy()
    assert np.isfinite(loss).all() and not flags.any()
    assert all(loss[a + A * second[a]] == min(loss[a], loss[a + A]) for a in range(A))      # the chosen hypothesis is the lower-loss one
    theta = fits.theta.cpu().numpy().astype(np.float64)
    for a, info in enumerate(st["proposals"].info):                              # reported, not asserted: how good the fit is from these starts
        m = np.nonzero(st["proposals"].clusters.label.cpu().numpy() == info["cluster"])[0]
        who = int(np.unique(sc["owner"][sc["mask"] != 0][m])[0])
        y_true, centre = sc["truth"][who]
        row = theta[a + A * second[a]]
        print("object %d: yaw error (mod pi) %.3f -> %.3f rad, front/back %s; centre error %.3f -> %.3f m; loss %.4e / %.4e" %
              (who, _yaw_error(info["yaw"], y_true), _yaw_error(row[0], y_true),
               "right" if abs((row[0] - y_true + np.pi) % (2 * np.pi) - np.pi) < np.pi / 2 else "WRONG",
               np.linalg.norm(info["centre"] - centre), np.linalg.norm(row[1:4] * row[4] - centre), loss[a], loss[a + A]))
