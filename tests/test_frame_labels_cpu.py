"""CPU tests of the host side of frame labelling (sdflabel_amd/frame.py, pipelines/refinement.py) against golden G18, recorded from the
reference's own utils/refinement.py functions (tools/make_golden_frame.py)."""
import numpy as np
import pytest
import torch

from sdflabel_amd import frame as FR
from sdflabel_amd.pipelines import refinement as rtools
from tests._util import gold


@pytest.fixture(scope="module")
def z():
    return gold("g18_frame_labels.npz")


@pytest.mark.parametrize("tag,dtype", [("f32", np.float32), ("f16", np.float16)])
def test_label_assembly_matches_the_reference(z, tag, dtype):
    """golden extents and parameters -> assemble_labels: location, rotation_y, alpha and cam_T within 1e-6 (1 ulp of float32 in cos / sin,
    amplified by at most 1 / |sin| <= 10 in the acos); dimensions bit-equal"""
    n = int(z["label_n"])
    assert n >= 6
    P = lambda k: np.stack([z["label%d_%s" % (i, k)] for i in range(n)])      # noqa: E731
    ext = np.stack([z["label%d_%s_ext" % (i, tag)] for i in range(n)])
    assert ext.dtype == dtype
    bboxes = [z["label%d_bbox" % i].tolist() for i in range(n)]
    labels, cam_T = FR.assemble_labels(ext, P("yaw").astype(dtype)[:, 0], P("trans").astype(dtype), P("scale").astype(dtype)[:, 0], z["label_p_WC"],
                                       bboxes)
    for i in range(n):
        q = "label%d_%s_" % (i, tag)
        lab = labels[i]
        assert abs(np.sin(z[q + "rotation_y"])) >= 0.1
        assert np.abs(lab["location"] - z[q + "location"]).max() < 1e-6
        assert abs(lab["rotation_y"] - float(z[q + "rotation_y"])) < 1e-6 and abs(lab["alpha"] - float(z[q + "alpha"])) < 1e-6
        assert np.abs(cam_T[i] - z[q + "cam_T"]).max() < 1e-6
        dims = np.asarray(lab["dimensions"])
        assert dims.dtype == dtype == z[q + "dimensions"].dtype and np.array_equal(dims, z[q + "dimensions"])
        assert lab["name"] == "Car" and lab["bbox"] == bboxes[i] and lab["score"] == int(z[q + "score"]) == 1
        assert lab["location"].dtype == np.float64 and isinstance(lab["rotation_y"], float)
    # one annotation alone gives the batch's values
    one, cT = FR.assemble_labels(ext[2:3], P("yaw").astype(dtype)[2:3, 0], P("trans").astype(dtype)[2:3], P("scale").astype(dtype)[2:3, 0],
                                 z["label_p_WC"], bboxes[2:3])
    assert np.abs(one[0]["location"] - labels[2]["location"]).max() < 1e-12 and one[0]["rotation_y"] == labels[2]["rotation_y"]


def test_bev_angles_match_the_reference(z):
    for pose, ry, al in zip(z["h_poses"], z["h_roty"], z["h_alpha"]):
        got = rtools.roty_in_bev(pose)
        assert isinstance(got, float) and got == ry
        assert rtools.alpha_in_bev(pose, got) == al
    bad = np.eye(4)
    bad[0, 2] = 1.0000001                                 # the reference's math.acos raises outside [-1, 1]
    with pytest.raises(ValueError):
        rtools.roty_in_bev(bad)


def test_box_ious_match_the_reference(z):
    for a, b, c, g in zip(z["h_boxA"], z["h_boxB"], z["h_compute_iou"], z["h_get_iou"]):
        assert rtools.compute_iou(list(a), list(b)) == c
        assert rtools.get_iou(list(a), list(b)) == g
    assert (z["h_get_iou"] == 0).any() and (z["h_get_iou"] > 0).any()
    assert rtools.get_iou([0, 0, 10, 10], [20, 20, 30, 30]) == 0.0 and rtools.compute_iou([0, 0, 9, 9], [0, 0, 9, 9]) == 1.0


def test_adjust_intrinsics_crop_and_rot_from_yaw_match_the_reference(z):
    for i in range(int(z["h_adj_n"])):
        l, t, r, b = z["h_adj%d_bbox" % i].tolist()
        size, intr, off = rtools.adjust_intrinsics_crop(z["h_K"], torch.Tensor([b - t, r - l]), (l, t, r, b), 32 ** 2)
        assert size == z["h_adj%d_size" % i].tolist() and isinstance(size, list)
        assert intr.dtype == off.dtype == torch.float32
        assert np.array_equal(intr.numpy(), z["h_adj%d_intrinsics" % i]) and np.array_equal(off.numpy(), z["h_adj%d_off" % i])
    for y, R in zip(z["h_yaws"], z["h_rot_from_yaw"]):
        got = rtools.rot_from_yaw(float(y))
        assert got.dtype == torch.float32 and np.abs(got.numpy() - R).max() <= 2.0 ** -23
    t = rtools.rot_from_yaw(torch.tensor([0.5], dtype=torch.float64))
    assert t.dtype == torch.float64 and t.shape == (3, 3)


def test_init_params_host_algebra_matches_the_reference(z):
    """refine_css.py:173-196 given the golden's extents: the constrained rotation and yaw, the IoU on both sides of 0.7, the height fix-up
    and trans = tra / scale"""
    n = int(z["init_n"])
    sides = set()
    for i in range(n):
        p = "init%d_" % i
        assert z[p + "iou_margin"] >= 1e-3
        scale = float(z[p + "scale"]) if bool(z[p + "scale_is_float"]) else np.float32(z[p + "scale"])
        pose = {"scale": scale, "rot": z[p + "rot"].copy(), "tra": z[p + "tra"].copy()}
        rot, yaw = FR.constrain_rotation(pose["rot"])
        assert np.array_equal(rot, z[p + "rot_constrained"]) and yaw == float(z[p + "yaw"])
        params, iou = FR.init_params_host(pose, rot, yaw, z[p + "ext"], z[p + "scene_ymin"], z[p + "bbox"].tolist(), z[p + "latent"])
        assert abs(iou - float(z[p + "iou"])) < 1e-6 and (iou < 0.7) == (float(z[p + "iou"]) < 0.7)
        sides.add(bool(iou < 0.7))
        assert params["trans"].dtype == z[p + "trans"].dtype and np.array_equal(params["trans"], z[p + "trans"])
        assert params["yaw"].shape == (1,) and params["yaw"][0] == float(z[p + "yaw"])
        assert params["scale"].shape == (1,) and params["scale"][0] == scale and np.array_equal(params["latent"], z[p + "latent"])
        assert np.array_equal(pose["rot"], z[p + "rot"]) and np.array_equal(pose["tra"], z[p + "tra"])        # the caller's pose is not modified
    assert sides == {True, False}


def test_frame_dict_stacks_the_labels(z):
    n = int(z["label_n"])
    labels = [{"name": "Car", "bbox": z["label%d_bbox" % i].tolist(), "location": z["label%d_f32_location" % i],
               "dimensions": list(z["label%d_f32_dimensions" % i]), "rotation_y": float(z["label%d_f32_rotation_y" % i]),
               "alpha": float(z["label%d_f32_alpha" % i]), "score": 1} for i in range(n)]
    d = FR.frame_dict([labels[0], None, (labels[1], None, None)] + labels[2:])
    assert d["name"] == ["Car"] * n
    assert d["location"].shape == (n, 3) and d["dimensions"].shape == (n, 3) and d["bbox"].shape == (n, 4)
    assert d["rotation_y"].shape == d["alpha"].shape == d["score"].shape == (n,)
    assert np.array_equal(d["dimensions"][1], z["label1_f32_dimensions"])
    e = FR.frame_dict([])
    assert e["name"] == [] and all(e[k].shape[0] == 0 for k in FR.NECESSARY_KEYS)


def test_no_cpu_fallback_for_the_point_arithmetic():
    from sdflabel_amd import _lib
    import sdflabel_amd
    with pytest.raises(_lib.SdfrError):
        FR.reproject_device([np.zeros((4, 5, 3), np.float32)], [np.ones((4, 5), np.float32)], [np.eye(3, dtype=np.float32)], device="cpu")
    with pytest.raises(_lib.SdfrError):
        FR.labels_many(None, sdflabel_amd.Grid3D(4), [], np.eye(4), [])
