"""cliqa on the HIP engine: the JPEG quality, grain noise and scale factor nets (``cliqa/models``, reference) and the patch
selection and ``predict_*`` functions of ``cliqa/utils.py``.  Kernels: nunif_amd/csrc/cliqa.hip."""
