"""``python -m compressai.utils.video.eval_model`` (reference: compressai/utils/video/eval_model/)."""
