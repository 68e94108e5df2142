"""``waifu2x.ui_utils.process_video`` on the HIP engine (``waifu2x/ui_utils.py:104-206``).

Only the per-frame callback changes: it comes from :class:`nunif_amd.waifu2x.video.Waifu2xVideoStream`; the config the reference's
``config_callback`` builds is marked as an engine callback's, and where the engine's ``configure_colorspace`` then records
``engine_pixfmt`` the stream takes the decoder's planes and returns the encoder's.  Output naming,
``--resume``, the overwrite prompt and ``config_callback`` stay the reference's own code: the reference function is run as it is,
over a copy of its module globals in which ``VU.process_video`` receives the engine's callbacks instead of the closure the
function built.  Bound by ``nunif_amd.install()``; without an installed reference there is nothing to delegate to.

The image route (``waifu2x/ui_utils.py:32-100``: ``make_output_filename``, ``process_image``, ``process_images``) stands on its own:
``process_image`` returns the device tensors ``Waifu2x.convert`` gives, and :class:`ImageWriter` turns them into the bytes of a
PNG file on the device (``nunif_amd/nunif/utils/png.py``) where the reference copies them to the host and runs libpng at level 6
on a thread pool (``nunif/utils/pil_io.py:240-323``).  What the device encoder does not write (webp, jpeg, 16-bit sources, ICC
profiles, frames beyond 8192, the wand image library) goes the reference's way through PIL.  ``install()`` does not bind these
three: an installed reference CLI keeps its own image route.
"""
import io
import os
import queue
import struct
import threading
import types
import warnings
from multiprocessing import cpu_count
from os import path

import numpy as np
import torch
from PIL import Image, ImageOps, PngImagePlugin, UnidentifiedImageError

from ..nunif.utils import png as PNG
from ..nunif.utils.rgb_noise import apply_rgb_noise, rgb_noise_like
from .video import Waifu2xVideoStream


class _VideoUtilsProxy:
    """The reference's ``nunif.utils.video`` module with ``process_video`` taking its frame callbacks from a stream."""

    def __init__(self, vu, make_stream):
        self._vu, self._make_stream = vu, make_stream

    def __getattr__(self, name):
        return getattr(self._vu, name)

    def process_video(self, input_path, output_path, frame_callback=None, config_callback=None, **kwargs):
        if frame_callback is None:
            raise RuntimeError("waifu2x.ui_utils.process_video no longer hands VU.process_video a frame_callback: the engine's "
                               "process_video does not fit this reference checkout")
        stream = self._make_stream()
        kwargs["test_callback"] = stream.test_callback(self._vu.to_frame)

        def engine_config_callback(video_stream):
            # the reference's own config, marked as belonging to an engine callback: the engine's configure_colorspace
            # (nunif_amd/nunif/utils/video.py) may then leave both pixel-format conversions to the stream, which reads
            # config.state["engine_pixfmt"] at its first frame
            config = (config_callback or self._vu.default_config_callback)(video_stream)
            if hasattr(stream, "bind_config"):
                stream.bind_config(config, vf=kwargs.get("vf", ""))
            return config

        return self._vu.process_video(input_path, output_path, frame_callback=stream.av_callback(self._vu.to_frame),
                                      config_callback=engine_config_callback, **kwargs)


def process_video(ctx, input_filename, output_path, args):
    from .. import install as inst
    ref = inst.original("waifu2x.ui_utils", "process_video")
    if ref is None:
        raise RuntimeError("nunif_amd.waifu2x.ui_utils.process_video runs underneath the reference's waifu2x.ui_utils: "
                           "call nunif_amd.install() first")
    # the substitution below rests on the reference spelling its call `VU.process_video(...)`: if it stops doing so its torch
    # frame callback would run again, silently — refuse instead
    vu = ref.__globals__.get("VU")
    if vu is None or not {"VU", "process_video"} <= set(ref.__code__.co_names) or not hasattr(vu, "process_video"):
        raise RuntimeError("waifu2x.ui_utils.process_video does not call VU.process_video any more: the engine's "
                           "process_video does not fit this reference checkout")
    ref_globals = dict(ref.__globals__)
    ref_globals["VU"] = _VideoUtilsProxy(vu, lambda: Waifu2xVideoStream(
        ctx, args, device=args.state["device"], use_16bit=vu.pix_fmt_requires_16bit(args.pix_fmt)))
    run = types.FunctionType(ref.__code__, ref_globals, ref.__name__, ref.__defaults__, ref.__closure__)
    run.__kwdefaults__ = ref.__kwdefaults__
    return run(ctx, input_filename, output_path, args)


# ---- the image route ------------------------------------------------------------------------------------------------------------------
SMB_INVALID_CHARS = '\\/:*?"<>|'
GAMMA_LCD = 45454                                                # nunif/utils/pil_io.py:23
IMAGE_IO_QUEUE_MAX = 100                                         # futures kept before the writer waits for them
LOAD_QUEUE_MAX = 128                                             # waifu2x/ui_utils.py:76 max_queue_size


def _set_image_ext(filename, format):
    """nunif/utils/filename.py:4-18: the extension goes first, whatever it was."""
    format = format.lower()
    stem = path.splitext(filename)[0]
    if format in {"png", "webp"}:
        return stem + "." + format
    if format in {"jpg", "jpeg"}:
        return stem + ".jpg"
    raise NotImplementedError(f"{format}")


def make_output_filename(input_filename, args, video=False):
    basename = path.basename(input_filename).translate({ord(c): ord("_") for c in SMB_INVALID_CHARS})
    if video:
        return path.splitext(basename)[0] + args.video_extension
    return _set_image_ext(basename, args.format)


def _image_cms(filename):
    try:
        from PIL import ImageCms
    except ImportError as e:
        raise RuntimeError(f"{filename}: the image carries an ICC profile and this PIL has no ImageCms (littlecms)") from e
    return ImageCms


def _icc_convert(im, icc_profile, filename, to_srgb, mode=None):
    """The profile step of ``pil_io._load_image`` (:54-73, ``to_srgb``) and of ``save_image`` (:263-285) for colour images;
    returns (image, whether the profile was applied).  Grey images would need the reference's CIE grey profile, which is not
    part of this tree: they keep their values, with a warning, as the reference does when littlecms refuses a profile."""
    ImageCms = _image_cms(filename)
    mode = mode or im.mode
    if mode in {"L", "LA"}:
        warnings.warn(f"{filename}: the ICC profile of a grey image is not applied")
        return im, False
    srgb = ImageCms.createProfile("sRGB")
    with io.BytesIO(icc_profile) as handle:
        try:
            other = ImageCms.ImageCmsProfile(handle)
            if to_srgb:
                if im.mode == "CMYK":
                    return ImageCms.profileToProfile(im, other, srgb, outputMode="RGB"), True
                return ImageCms.profileToProfile(im, other, srgb), True
            if mode == "CMYK":
                return ImageCms.profileToProfile(im, srgb, other, outputMode="CMYK").convert("RGB"), True
            return ImageCms.profileToProfile(im, srgb, other), True
        except ImageCms.PyCMSError as e:
            warnings.warn(f"{filename}: profile error: im.mode={im.mode}, {e}")
            return im, False


def _prepare_image(im, filename, exif_transpose=False):
    """``pil_io._load_image(im, filename, color="rgb", keep_alpha=True)`` (:38-123), the arguments ``process_images`` gives it:
    -> (PIL image in RGB, RGBA, I or I;16; meta)."""
    meta = {"engine": "pil", "filename": filename}
    im.load()
    if exif_transpose:
        ImageOps.exif_transpose(im, in_place=True)
    meta["mode"] = im.mode
    if im.mode in {"L", "I", "RGB", "P"}:
        transparency = im.info.get("transparency")
        if isinstance(transparency, (bytes, int)):               # tRNS -> alpha
            if im.mode in {"RGB", "P"}:
                im = im.convert("RGBA")
            elif im.mode == "L":
                im = im.convert("LA")
    meta["icc_profile"] = im.info.get("icc_profile")
    if meta["icc_profile"] is not None:
        im, _ = _icc_convert(im, meta["icc_profile"], filename, to_srgb=True)
    if im.mode not in {"RGB", "RGBA", "L", "LA", "I", "I;16"}:
        im = im.convert("RGB")
    meta["depth"] = 8 if im.mode not in {"I", "I;16"} else 16
    meta["grayscale"] = im.mode in {"L", "LA", "I", "I;16"}
    meta["gamma"] = None
    gamma = im.info.get("gamma")
    if gamma is not None:
        gamma = int(float(gamma) * 100000)
        if gamma != 0 and gamma != GAMMA_LCD:
            meta["gamma"] = gamma
    if im.mode == "L":
        im = im.convert("RGB")
    elif im.mode == "LA":
        im = im.convert("RGBA")
    return im, meta


def load_image(filename, exif_transpose=False):
    """``pil_io.load_image`` (:172-190) for the image route; (None, None) for a file PIL cannot open."""
    try:
        with open(filename, "rb") as f:
            return _prepare_image(Image.open(f), filename, exif_transpose=exif_transpose)
    except (UnidentifiedImageError, Image.DecompressionBombError, OSError, ValueError, SyntaxError):
        return None, None


def to_tensor(im):
    """``pil_io.to_tensor(im, return_alpha=True)`` (:218-237): -> (float [C,H,W] in 0..1, alpha [1,H,W] or None) on the host."""
    alpha = None
    if im.mode in {"RGBA", "LA"}:
        alpha = im.getchannel("A")
        im = im.convert(im.mode[:-1])

    def planes(image):
        a = np.array(image)
        x = torch.from_numpy(a if a.ndim == 3 else a[:, :, None]).permute(2, 0, 1)
        if x.dtype == torch.uint16:
            return x.to(torch.int32).float() / 65535
        if x.dtype != torch.float32:
            return x.float() / torch.iinfo(x.dtype).max
        return x
    return planes(im).contiguous(), (planes(alpha).contiguous() if alpha is not None else None)


def quantize256(x):
    """nunif/transforms/functional.py:9-12"""
    return torch.clamp((x * 255).round_(), 0, 255).to(torch.uint8)


def to_image(rgb, alpha=None, depth=None):
    """``pil_io.to_image`` (:240-253) on host tensors, for the files PIL writes."""
    if depth == 16:                                              # PIL has no 16-bit RGB: 16-bit grey
        if rgb.shape[0] != 1:
            rgb = rgb.mean(dim=0, keepdim=True)
        im = Image.fromarray((rgb * 0xffff).to(torch.int16).numpy().astype(np.uint16)[0])
    else:
        q = quantize256(rgb).permute(1, 2, 0).contiguous().numpy()
        im = Image.fromarray(q[:, :, 0], "L") if q.shape[2] == 1 else Image.fromarray(q, "RGB")
    if alpha is not None:
        im.putalpha(Image.fromarray(quantize256(alpha)[0].contiguous().numpy(), "L"))
    return im


def save_image(im, filename, format="png", meta=None, bg_color=255):
    """``pil_io.save_image`` (:256-323) for the PIL engine."""
    icc_profile = None
    if meta is not None:
        assert meta["engine"] == "pil"
        if meta["icc_profile"] is not None:
            if meta["mode"] in {"L", "LA"} and im.mode in {"RGB", "RGBA"}:
                im = im.convert(meta["mode"])
            im, applied = _icc_convert(im, meta["icc_profile"], str(filename), to_srgb=False, mode=meta["mode"])
            icc_profile = meta["icc_profile"] if applied else None
        if meta["grayscale"]:
            if im.mode == "RGB":
                im = im.convert("L")
            elif im.mode == "RGBA":
                im = im.convert("LA")
    if format == "png":
        pnginfo = PngImagePlugin.PngInfo()
        if meta is not None and meta["gamma"] is not None:
            pnginfo.add(b"gAMA", struct.pack(">I", meta["gamma"]))
        options = {"icc_profile": icc_profile, "pnginfo": pnginfo, "compress_level": 6}
    elif format == "webp":
        options = {"icc_profile": icc_profile, "quality": 95, "method": 4, "lossless": True}
    elif format in {"jpg", "jpeg"}:
        format = "jpeg"
        options = {"icc_profile": icc_profile, "quality": 95, "subsampling": "4:4:4"}
        if im.mode in {"LA", "RGBA"}:
            nobg = Image.new(im.mode[:-1], im.size, tuple([bg_color] * (len(im.mode) - 1)))
            nobg.paste(im, im.getchannel("A"))
            im = nobg
            warnings.warn(f"{filename}: alpha channel is removed")
    else:
        raise NotImplementedError(f"{format}")
    im.save(filename, format=format, **options)


@torch.inference_mode()
def process_image(ctx, im, meta, args):
    """``waifu2x/ui_utils.py:41-71`` up to the copy to the host: -> (rgb [3,H,W], alpha [1,H,W] or None), device tensors for
    :class:`ImageWriter`.  ``meta`` takes ``depth`` and ``grayscale`` from ``args`` as in the reference."""
    if args.rotate_left:
        im = im.transpose(Image.Transpose.ROTATE_90)
    elif args.rotate_right:
        im = im.transpose(Image.Transpose.ROTATE_270)
    rgb, alpha = to_tensor(im)
    if rgb.shape[0] == 1:
        rgb = rgb.repeat(3, 1, 1)
    device = args.state["device"]
    rgb, alpha = ctx.convert(rgb, alpha, args.method, args.noise_level, args.tile_size, args.batch_size, args.tta,
                             enable_amp=not args.disable_amp, output_device=device)
    if args.grain:
        noise = rgb_noise_like(rgb)
        rgb = apply_rgb_noise(rgb, noise, strength=args.grain_strength * 0.5)      # grain_strength = 1/2 for image
    if alpha is not None:
        alpha = alpha.to(device)
    if getattr(args, "depth", None) is not None and getattr(args, "image_lib", "pil") == "wand":
        meta["depth"] = args.depth
    if args.grayscale:
        meta["grayscale"] = True
    return rgb, alpha


def _write_bytes(file_path, data):
    with open(file_path, "wb") as f:
        f.write(data)


def _save_with_pil(rgb, alpha, depth, file_path, meta, format):
    save_image(to_image(rgb, alpha, depth=depth), file_path, format=format, meta=meta)


class ImageWriter():
    """``write(rgb, alpha, meta, output_filename)``: the file of one converted image.  A PNG of 8 bits without an ICC profile
    and within the encoder's 8192 x 8192 is encoded on the device, one :class:`PngEncoder` per device under a lock, and the pool
    only writes its bytes; everything else becomes the PIL image the reference makes and is saved by PIL on the pool."""

    def __init__(self, output_dir, pool, args):
        self.output_dir, self.pool, self.args = output_dir, pool, args
        self.futures = []
        self._encoders = {}
        self._lock = threading.Lock()

    @staticmethod
    def uses_device_encoder(format, depth, icc_profile, H, W, image_lib="pil"):
        return (format == "png" and depth == 8 and icc_profile is None and H <= PNG.MAX_DIM and W <= PNG.MAX_DIM
                and image_lib != "wand")

    def _encoder(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._encoders:
            self._encoders[device] = PNG.PngEncoder(device)
        return self._encoders[device]

    def drain(self):
        for f in self.futures:
            f.result()
        self.futures.clear()

    def write(self, rgb, alpha, meta, output_filename):
        args = self.args
        depth = meta["depth"] if meta.get("depth") is not None else 8
        H, W = rgb.shape[-2:]
        if self.uses_device_encoder(args.format, depth, meta["icc_profile"], H, W, getattr(args, "image_lib", "pil")):
            if alpha is not None:
                alpha = alpha.to(rgb.device)
            with self._lock:
                data = self._encoder(rgb.device).encode(rgb, alpha=alpha, gray=bool(meta["grayscale"]), gamma=meta["gamma"])
            self.futures.append(self.pool.submit(_write_bytes, output_filename, data))
        else:
            self.futures.append(self.pool.submit(_save_with_pil, rgb.cpu(), alpha.cpu() if alpha is not None else None, depth,
                                                 output_filename, meta, args.format))
        if len(self.futures) >= IMAGE_IO_QUEUE_MAX:
            self.drain()


def _load_ahead(files, exif_transpose, q, stop):
    for filename in files:
        if stop.is_set():
            break
        q.put(load_image(filename, exif_transpose=exif_transpose))
    q.put(None)


def _tqdm():
    try:
        from tqdm import tqdm
        return tqdm
    except ImportError:
        class Bar():
            def __init__(self, *a, **k):
                pass

            def update(self, n=1):
                pass

            def close(self):
                pass
        return Bar


def process_images(ctx, files, output_dir, args, title=None):
    """``waifu2x/ui_utils.py:74-100``: the files load on a thread ahead of the GPU, the device encodes, the pool writes."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(output_dir, exist_ok=True)
    q, stop = queue.Queue(maxsize=LOAD_QUEUE_MAX), threading.Event()
    loader = threading.Thread(target=_load_ahead, args=(list(files), not args.disable_exif_transpose, q, stop), daemon=True)
    loader.start()
    try:
        with ThreadPoolExecutor(max_workers=cpu_count() // 2 or 1) as pool:
            writer = ImageWriter(output_dir, pool, args)
            pbar = (args.state["tqdm_fn"] or _tqdm())(ncols=80, total=len(files), desc=title)
            while True:
                item = q.get()
                if item is None:
                    break
                im, meta = item
                if im is None:                                   # a file PIL cannot open
                    continue
                output_filename = path.join(output_dir, make_output_filename(meta["filename"], args, video=False))
                if args.resume and path.exists(output_filename):
                    continue
                rgb, alpha = process_image(ctx, im, meta, args)
                writer.write(rgb, alpha, meta, output_filename)
                pbar.update(1)
                if args.state["stop_event"] is not None and args.state["stop_event"].is_set():
                    break
            writer.drain()
            pbar.close()
    finally:
        stop.set()
        while loader.is_alive():                                 # let a loader that waits for room in the queue end
            try:
                q.get(timeout=0.05)
            except queue.Empty:
                pass
        loader.join()
