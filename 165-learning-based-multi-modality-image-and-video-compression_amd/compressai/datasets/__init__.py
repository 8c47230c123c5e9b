"""Datasets (reference: compressai/datasets/__init__.py:30-40).

Still images: the plain ``ImageFolder`` and the paired FLIR RGB + thermal loaders.  Video: ``VideoFolder``
(training clips from frame folders) and ``RawVideoSequence`` (memory-mapped raw ``.yuv`` files, what
``compressai.utils.video.eval_model`` reads).
"""
from .image import TEST_TRANSFORM, TRAIN_TRANSFORM, ImageFolder
from .image_rgbt import (FLIR_TEST_LIST, ImageFolderRGB, ImageFolderT, ImageFolderTest, guided_dir,
                         paired_random_crop, paired_train_transforms)
from .rawvideo import RawVideoSequence, VideoFormat, get_raw_video_file_info
from .video import VideoFolder

__all__ = ["ImageFolder", "ImageFolderRGB", "ImageFolderT", "ImageFolderTest", "TEST_TRANSFORM",
           "TRAIN_TRANSFORM", "FLIR_TEST_LIST", "guided_dir", "paired_random_crop", "paired_train_transforms",
           "RawVideoSequence", "VideoFormat", "get_raw_video_file_info", "VideoFolder"]
