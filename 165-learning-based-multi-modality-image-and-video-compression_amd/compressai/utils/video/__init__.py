"""Video evaluation utilities (reference: compressai/utils/video/): the fused per-frame ops (``frames``) and
``python -m compressai.utils.video.eval_model``."""
