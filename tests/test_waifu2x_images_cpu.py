"""The waifu2x image route (nunif_amd/waifu2x/ui_utils.py) without a GPU: the three public functions keep the reference's
signatures; the in-tree loader answers the ``meta`` the reference's ``pil_io.load_image`` recorded for the same files
(tests/golden/waifu2x_image_meta.json), the tRNS conversion and the gamma rule included; the output names; the PIL restatements
``to_tensor`` / ``to_image`` / ``save_image``; and the table of what the writer sends to the device encoder."""
import inspect
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

import waifu2x_image_sources as S
from conftest import GOLDEN
from oracle import refstub


def test_signatures_equal_the_reference():
    if not refstub.reference_available():
        pytest.skip("/root/reference is not mounted here")
    refstub.install()
    import waifu2x.ui_utils as ref
    from nunif_amd.waifu2x import ui_utils as U
    for name in ("process_image", "process_images", "make_output_filename"):
        assert inspect.signature(getattr(U, name)) == inspect.signature(getattr(ref, name)), name


def test_output_names():
    from nunif_amd.waifu2x.ui_utils import make_output_filename
    args = SimpleNamespace(format="png", video_extension=".mp4")
    assert make_output_filename("/a/b/c.jpeg", args) == "c.png"
    assert make_output_filename('x:y*z?"<>|.webp', args) == "x_y_z_____.png"
    assert make_output_filename("/a/clip.mkv", args, video=True) == "clip.mp4"
    assert make_output_filename("c.png", SimpleNamespace(format="jpeg")) == "c.jpg"
    assert make_output_filename("c.tar.png", SimpleNamespace(format="webp")) == "c.tar.webp"
    with pytest.raises(NotImplementedError):
        make_output_filename("c.png", SimpleNamespace(format="bmp"))


def test_the_loader_answers_the_reference_meta(tmp_path):
    from nunif_amd.waifu2x.ui_utils import load_image
    want = json.load(open(os.path.join(GOLDEN, "waifu2x_image_meta.json")))
    for gamma in (None, 0.5, 0.45454):
        d = tmp_path / str(gamma)
        d.mkdir()
        for mode, f in S.write_sources(d, gamma=gamma).items():
            im, meta = load_image(f, exif_transpose=True)
            got = dict(meta, filename=os.path.basename(meta["filename"]), loaded_mode=im.mode)
            assert got == want[f"{mode}/gamma={gamma}"], (mode, gamma)
    assert want["P/gamma=None"]["loaded_mode"] == "RGBA" and want["L/gamma=0.5"]["gamma"] == 50000
    assert want["RGB/gamma=0.45454"]["gamma"] is None                     # the LCD gamma is dropped
    bad = tmp_path / "bad.png"
    bad.write_bytes(b"not an image")
    assert load_image(str(bad)) == (None, None) and load_image(str(tmp_path / "missing.png")) == (None, None)


def test_to_tensor_to_image_and_save_image(tmp_path):
    from nunif_amd.waifu2x import ui_utils as U
    im = S.source_image("RGBA", 1)
    rgb, alpha = U.to_tensor(im)
    a = np.asarray(im)
    assert rgb.shape == (3, S.H, S.W) and alpha.shape == (1, S.H, S.W) and rgb.dtype == torch.float32
    assert torch.equal(rgb, torch.from_numpy(a[..., :3].copy()).permute(2, 0, 1).float() / 255)
    assert np.array_equal(np.asarray(U.to_image(rgb, alpha)), a)          # 8 bits: a round trip
    grey, none = U.to_tensor(S.source_image("L", 2))
    assert grey.shape == (1, S.H, S.W) and none is None
    x = torch.rand(3, 8, 9, generator=torch.Generator().manual_seed(3)) * 1.4 - 0.2
    assert torch.equal(U.quantize256(x), torch.clamp((x * 255).round(), 0, 255).to(torch.uint8))
    im16 = U.to_image(torch.full((3, 4, 5), 0.25), depth=16)
    assert im16.mode in ("I;16", "I;16L", "I;16N") and int(np.asarray(im16)[0, 0]) == int(0.25 * 0xffff)
    meta = {"engine": "pil", "filename": "f", "mode": "L", "icc_profile": None, "depth": 8, "grayscale": True, "gamma": 50000}
    out = str(tmp_path / "o.png")
    U.save_image(U.to_image(rgb, alpha), out, format="png", meta=meta)
    with Image.open(out) as back:
        assert back.mode == "LA" and back.info["gamma"] == 0.5
        assert np.array_equal(np.asarray(back), np.asarray(Image.fromarray(a, "RGBA").convert("LA")))
    for fmt, ext, mode in (("webp", "webp", "RGBA"), ("jpeg", "jpg", "RGB")):
        out = str(tmp_path / ("o." + ext))
        with pytest.warns(UserWarning) if fmt == "jpeg" else _nothing():
            U.save_image(U.to_image(rgb, alpha), out, format=fmt, meta=dict(meta, grayscale=False))
        with Image.open(out) as back:
            assert back.mode == mode and back.size == (S.W, S.H)


class _nothing():
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def test_the_routing_table():
    """What goes to the device encoder: PNG, 8 bits, no ICC profile, at most 8192 x 8192, the PIL image library."""
    from nunif_amd.waifu2x.ui_utils import ImageWriter
    use = ImageWriter.uses_device_encoder
    table = {("png", 8, None, 40, 56): True, ("png", 8, None, 8192, 8192): True,
             ("png", 8, None, 8193, 56): False, ("png", 8, None, 40, 8193): False,
             ("png", 16, None, 40, 56): False, ("png", 8, b"icc", 40, 56): False,
             ("webp", 8, None, 40, 56): False, ("jpeg", 8, None, 40, 56): False, ("jpg", 8, None, 40, 56): False}
    for (fmt, depth, icc, H, W), want in table.items():
        assert use(fmt, depth, icc, H, W) is want, (fmt, depth, icc, H, W)
    assert use("png", 8, None, 40, 56, image_lib="wand") is False
