"""``waifu2x.ui_utils.process_video`` on the HIP engine (``waifu2x/ui_utils.py:104-206``).

Only the per-frame callback changes: it comes from :class:`nunif_amd.waifu2x.video.Waifu2xVideoStream`; the config the reference's
``config_callback`` builds is marked as an engine callback's, and where the engine's ``configure_colorspace`` then records
``engine_pixfmt`` the stream takes the decoder's planes and returns the encoder's.  Output naming,
``--resume``, the overwrite prompt and ``config_callback`` stay the reference's own code: the reference function is run as it is,
over a copy of its module globals in which ``VU.process_video`` receives the engine's callbacks instead of the closure the
function built.  Bound by ``nunif_amd.install()``; without an installed reference there is nothing to delegate to.
"""
import types

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
