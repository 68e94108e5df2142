"""The per-frame part of ``python -m iw3.desktop`` (reference) that runs on the HIP engine: the JPEG encoding of a streamed frame."""
