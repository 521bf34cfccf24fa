"""scene_viewer's `--skybox DIR` without a GPU: the flag, the six file names of the reference's example and their layer order."""
import argparse

import numpy as np
import pytest

from rend3_amd import scene_viewer as sv


def _write_faces(directory, size=4, ext=".png", skip=None):
    from PIL import Image
    for k, name in enumerate(sv.SKYBOX_FACES):
        if name == skip:
            continue
        img = np.zeros((size, size, 3), dtype=np.uint8)
        img[..., 0] = 10 + k          # the layer
        img[0, 1] = (1, 2, 3)         # row 0, column 1: the orientation
        Image.fromarray(img).save(str(directory / (name + ext)))


def test_flag_reaches_the_settings():
    ap = sv.add_arguments(argparse.ArgumentParser())
    ap.add_argument("scene")
    assert sv.settings_from(ap.parse_args(["x.glb"]))["skybox"] is None
    assert sv.settings_from(ap.parse_args(["x.glb", "--skybox", "sky"]))["skybox"] == "sky"
    assert sv.default_settings()["skybox"] is None


def test_faces_load_in_layer_order(tmp_path):
    assert sv.SKYBOX_FACES == ("right", "left", "top", "bottom", "front", "back")  # +X, -X, +Y, -Y, +Z, -Z
    _write_faces(tmp_path)
    faces = sv.load_skybox(str(tmp_path))
    assert faces.shape == (6, 4, 4, 4) and faces.dtype == np.uint8
    assert faces[:, 3, 3, 0].tolist() == [10, 11, 12, 13, 14, 15]
    assert (faces[:, 0, 1, :3] == (1, 2, 3)).all() and (faces[..., 3] == 255).all()


def test_missing_or_unequal_faces_are_errors(tmp_path):
    _write_faces(tmp_path, skip="bottom")
    with pytest.raises(FileNotFoundError, match="bottom"):
        sv.load_skybox(str(tmp_path))
    from PIL import Image
    Image.fromarray(np.zeros((4, 8, 3), dtype=np.uint8)).save(str(tmp_path / "bottom.png"))
    with pytest.raises(ValueError):
        sv.load_skybox(str(tmp_path))


def test_build_binds_the_cube(tmp_path):
    """build() uploads the faces as an sRGB cube and binds it; a renderer without cube textures raises instead of skipping"""
    _write_faces(tmp_path)
    calls = []

    class Stop(Exception):
        pass

    class R:
        handedness = sv.RIGHT

        def add_texture_cube(self, faces, srgb=True):
            calls.append(("cube", faces.shape, srgb))
            return 5

        def set_background_texture(self, handle):
            calls.append(("bind", handle))
            raise Stop

    settings = sv.default_settings(file="unused.glb", skybox=str(tmp_path))
    with pytest.raises(Stop):
        sv.build(R(), None, None, settings)
    assert calls == [("cube", (6, 4, 4, 4), True), ("bind", 5)]

    class NoCubes:
        handedness = sv.RIGHT

    with pytest.raises(AttributeError):
        sv.build(NoCubes(), None, None, settings)


@pytest.mark.gpu
def test_gpu_viewer_scene_with_a_skybox(tmp_path):
    """the reference's static_gltf asset through the harness with `--skybox`: six PNG faces of one 0 / 255 colour, so the frame
    is the oracle's with that clear colour (the identity tests/test_skybox.py rests on), sets and keys included"""
    import os

    import torch
    assert torch.cuda.is_available()
    from PIL import Image

    import rend3_amd as r3
    from oracle import host as oh
    from oracle.world import OracleRenderer
    from oracle.world import material_record as omk
    from test_gpu_parity import compare_frames
    for name in sv.SKYBOX_FACES:
        img = np.zeros((4, 4, 3), dtype=np.uint8)
        img[...] = (0, 255, 255)
        Image.fromarray(img).save(str(tmp_path / (name + ".png")))
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ap = sv.add_arguments(argparse.ArgumentParser())
    ap.add_argument("file")
    flags = ["--directional-light", "-1,-4,2", "--directional-light-intensity", "4", "--shadow-distance", "20", "--camera", "3,3,5,-0.55,-0.5"]
    argv = sv.normalize_argv([os.path.join(gold, "static_gltf-data.glb")] + flags)
    plain = sv.settings_from(ap.parse_args(argv))
    with_sky = sv.settings_from(ap.parse_args(argv + ["--skybox", str(tmp_path)]))
    w, h = 320, 180
    f32 = np.float32
    o, p = OracleRenderer(oh.RIGHT, f32(w) / f32(h)), r3.Renderer(oh.RIGHT, f32(w) / f32(h))
    io, ip = sv.build(o, oh, omk, plain), sv.build(p, r3.host, r3.material_record, with_sky)
    for k in range(2):
        fo = o.render(w, h, samples=io["samples"], ambient=io["ambient"], clear_color=(0.0, 1.0, 1.0, 1.0))
        fp = p.render(w, h, samples=ip["samples"], ambient=ip["ambient"], clear_color=ip["clear"])
        compare_frames(fo, fp, f"viewer with a skybox, frame {k}")
        assert (fo["vis"] == 0).sum() > 1000 and (fo["vis"] != 0).sum() > 1000
    assert p.stage_times()["skybox"][1] == 2
    p.close()
