"""Shot boundary detection on the HIP engine (``nunif/utils/shot_boundary_detection.py``, reference).

:class:`BoundaryDetector` is the reference's windowing (``detect_boundary`` :41-108) without the decoder around it: frames come in
through ``push`` in batches of at most ``padding_size``, stay on the device, and each window costs one device-to-host copy of
its kept predictions.  :func:`detect_boundary` has the reference's signature and decodes through the reference's own
``nunif.utils.video`` (PyAV); without the reference there is no decoder and it refuses.
"""
import torch

from .transnetv2 import TransNetV2


class BoundaryDetector:
    """``push(frames [n<=padding_size,3,27,48], pts)`` per decoded batch, then ``finish()`` -> set of pts.  A pts in the set is the
    END of a segment (:110).  ``model`` is a :class:`TransNetV2` (its fused ``predict``) or any callable returning
    ``(one_hot, ...)`` like the reference's."""

    def __init__(self, model, window_size=100, padding_size=25, threshold=0.5):
        assert (window_size % padding_size == 0 and
                window_size // padding_size >= 3)  # pad1 + frames + pad2
        self.model = model
        self.window_size, self.padding_size, self.threshold = window_size, padding_size, threshold
        self.chunks = []          # [(frames [padding_size,3,27,48], pts [padding_size] long, CPU)]
        self.results = []         # [(pred [kept] CPU, pts [kept] CPU)]
        self.frame_count = 0

    def _probabilities(self, x):
        if hasattr(self.model, "predict"):
            return self.model.predict(x).flatten()
        with torch.inference_mode():
            one_hot = self.model(x)
            if isinstance(one_hot, tuple):
                one_hot = one_hot[0]
            return torch.sigmoid(one_hot).flatten()

    def _window(self):
        p = self.padding_size
        x = torch.cat([x_ for x_, _ in self.chunks], dim=0)
        pts = torch.cat([pts_ for _, pts_ in self.chunks], dim=0)
        pred = self._probabilities(x)
        self.results.append((pred[p:-p].cpu(), pts[p:-p]))
        del self.chunks[:(self.window_size - p * 2) // p]

    def push(self, frames, pts):
        p = self.padding_size
        n = frames.shape[0]
        if n < 1 or n > p:
            raise ValueError(f"BoundaryDetector.push takes 1..{p} frames per call, got {n}")
        self.frame_count += n
        pts = torch.as_tensor(pts, dtype=torch.long).cpu()
        if n < p:
            frames = torch.cat((frames,) + (frames[-1:],) * (p - n), dim=0)
            pts = torch.cat((pts,) + (pts[-1:],) * (p - n), dim=0)
        if not self.chunks and not self.results:
            self.chunks.append((torch.cat((frames[0:1],) * p, dim=0), torch.cat((pts[0:1],) * p, dim=0)))
        self.chunks.append((frames, pts))
        if len(self.chunks) == self.window_size // p:
            self._window()

    def finish(self):
        if not self.chunks:
            return set()
        p = self.padding_size
        last_x, last_pts = self.chunks[-1][0][-1:], self.chunks[-1][1][-1:]
        pad_x, pad_pts = torch.cat((last_x,) * p, dim=0), torch.cat((last_pts,) * p, dim=0)
        while not self.results or self.results[-1][1][-1] != last_pts[0]:
            self.chunks.append((pad_x, pad_pts))
            if len(self.chunks) == self.window_size // p:
                self._window()
        preds = torch.cat([pred for pred, _ in self.results], dim=0)[:self.frame_count]
        pts = torch.cat([pts_ for _, pts_ in self.results], dim=0)[:self.frame_count]
        return set(pts[preds > self.threshold].tolist())


def _reference_video_utils():
    try:
        import importlib
        return importlib.import_module("nunif.utils.video")
    except Exception as e:
        raise RuntimeError("nunif_amd detect_boundary decodes through the reference's nunif.utils.video (PyAV): put the nunif "
                           f"checkout on sys.path ({e!r}); BoundaryDetector takes frames from any other decoder") from e


def detect_boundary(
        video_file,
        device="cuda",
        window_size=100, padding_size=25, threshold=0.5,
        max_fps=None,
        start_time=None,
        end_time=None,
        stop_event=None,
        suspend_event=None,
        tqdm_fn=None,
        tqdm_title=None,
):
    VU = _reference_video_utils()
    model = TransNetV2().load().eval().to(device)
    detector = BoundaryDetector(model, window_size=window_size, padding_size=padding_size, threshold=threshold)

    def config_callback(stream):
        if max_fps is None:
            return VU.VideoOutputConfig(fps=None)          # keep original frame rate, use raw pts
        fps = VU.get_fps(stream)
        if float(fps) > max_fps:
            fps = max_fps
        return VU.VideoOutputConfig(fps=fps)

    callback_pool = VU.FrameCallbackPool(
        detector.push,
        require_pts=True,
        batch_size=padding_size,
        device=device,
        max_workers=0,  # must be sequential
    )
    VU.hook_frame(
        video_file, callback_pool,
        config_callback=config_callback,
        title=tqdm_title or "Shot Boundary Detection",
        vf="scale=48:27:flags=bilinear",  # input size for TransNetV2
        start_time=start_time, end_time=end_time,
        stop_event=stop_event,
        suspend_event=suspend_event,
        tqdm_fn=tqdm_fn
    )
    if stop_event is not None and stop_event.is_set():
        return set()
    return detector.finish()
