"""Training clips from frame folders (reference: compressai/datasets/video.py), the Vimeo-90k layout:

    root/train.list, root/test.list      one folder name per line
    root/sequences/<name>/*.png          the frames of one clip, in file-name order

``dataset[i]`` is a tuple of ``max_frames`` frames.  The frames are concatenated along the channel axis, passed
through ``transform`` once (so a random crop or flip hits every frame alike) and split again.
"""
import random
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import Dataset

__all__ = ["VideoFolder"]


class VideoFolder(Dataset):
    """Args:
        root (str): the dataset's root directory
        rnd_interval (bool): draw the frame step from 1 .. (frames + 2) // max_frames instead of 1
        rnd_temp_order (bool): reverse the clip with probability 1/2
        transform (callable): takes the [H, W, 3 max_frames] uint8 array, returns a [3 max_frames, h, w] tensor
        split (str): ``'train'`` or ``'test'``: the list file to read
        max_frames (int): frames per sample
    """

    def __init__(self, root, rnd_interval=False, rnd_temp_order=False, transform=None, split="train", max_frames=3):
        if transform is None:
            raise RuntimeError("Transform must be applied")
        splitfile = Path(root) / f"{split}.list"
        splitdir = Path(root) / "sequences"
        if not splitfile.is_file():
            raise RuntimeError(f'Invalid file "{root}"')
        if not splitdir.is_dir():
            raise RuntimeError(f'Invalid directory "{root}"')
        with open(splitfile, "r") as f:
            self.sample_folders = [splitdir / line.strip() for line in f if line.strip()]
        self.max_frames = int(max_frames)
        self.rnd_interval = rnd_interval
        self.rnd_temp_order = rnd_temp_order
        self.transform = transform

    def __getitem__(self, index):
        from PIL import Image

        folder = self.sample_folders[index]
        samples = sorted(f for f in folder.iterdir() if f.is_file())
        max_interval = (len(samples) + 2) // self.max_frames
        interval = random.randint(1, max_interval) if self.rnd_interval else 1
        paths = samples[::interval][: self.max_frames]
        frames = np.concatenate([np.asarray(Image.open(p).convert("RGB")) for p in paths], axis=-1)
        frames = torch.chunk(self.transform(frames), self.max_frames)
        if self.rnd_temp_order and random.random() < 0.5:
            return frames[::-1]
        return frames

    def __len__(self):
        return len(self.sample_folders)
