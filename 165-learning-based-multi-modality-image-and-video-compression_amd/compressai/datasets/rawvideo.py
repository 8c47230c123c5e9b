"""Raw planar video files (reference: compressai/datasets/rawvideo.py).

``RawVideoSequence.from_file`` memory-maps a ``.yuv`` file and yields one structured ``(y, u, v)`` record per
frame; size, frame rate, bit depth and chroma format come from the file name (the Vooya convention
``name_WIDTHxHEIGHT[_FPS(Hz|fps)][_BITSbit][_P420|...]``, and the GStreamer / ffmpeg format strings such as
``I420_10LE`` or ``yuv420p10le``) unless given.  8-bit files hold ``uint8`` samples, deeper ones 16-bit
containers.  The frame count is file bytes // frame bytes, with the sample size applied to every plane.
"""
import enum
import os
import re
from fractions import Fraction
from typing import Any, Dict, Optional, Sequence, Union

import numpy as np

__all__ = ["VideoFormat", "RawVideoSequence", "get_raw_video_file_info"]


class VideoFormat(enum.Enum):
    YUV400 = "yuv400"   # planar 4:0:0
    YUV420 = "yuv420"   # planar 4:2:0
    YUV422 = "yuv422"   # planar 4:2:2
    YUV444 = "yuv444"   # planar 4:4:4
    RGB = "rgb"         # planar 4:4:4 RGB


# format tags of Vooya, GStreamer and ffmpeg, lower case
_FORMAT_TAGS = {
    "yuv400": VideoFormat.YUV400,
    "yuv420": VideoFormat.YUV420, "420": VideoFormat.YUV420, "p420": VideoFormat.YUV420, "i420": VideoFormat.YUV420,
    "yuv422": VideoFormat.YUV422, "p422": VideoFormat.YUV422, "i422": VideoFormat.YUV422, "y42b": VideoFormat.YUV422,
    "yuv444": VideoFormat.YUV444, "p444": VideoFormat.YUV444, "y444": VideoFormat.YUV444,
}
_NTSC_RATES = {"23.98": Fraction(24000, 1001), "23.976": Fraction(24000, 1001), "29.97": Fraction(30000, 1001),
               "59.94": Fraction(60000, 1001)}
_EXTENSIONS = ("yuv", "rgb", "raw")
# (horizontal, vertical) chroma divisors; 0: no chroma planes
_SUBSAMPLING = {VideoFormat.YUV400: (0, 0), VideoFormat.YUV420: (2, 2), VideoFormat.YUV422: (2, 1),
                VideoFormat.YUV444: (1, 1), VideoFormat.RGB: (1, 1)}
_SAMPLE_TYPES = {8: np.uint8, 10: np.uint16, 12: np.uint16, 14: np.uint16, 16: np.uint16}

_TAGS_RE = "|".join(sorted(_FORMAT_TAGS, key=len, reverse=True))
_PATTERNS = (
    r"(?P<width>\d+)x(?P<height>\d+)",
    r"(?P<framerate>[\d\.]+)(?:Hz|fps)",
    r"(?P<bitdepth>\d+)bit",
    rf"(?i:(?P<format>{_TAGS_RE}))(?:[p_]?(?P<bitdepth2>\d+)(?P<endianness>LE|BE|le|be))?",
    rf"(?P<extension>{'|'.join(_EXTENSIONS)})",
)


def _as_format(value) -> VideoFormat:
    if isinstance(value, VideoFormat):
        return value
    try:
        return _FORMAT_TAGS[str(value).lower()]
    except KeyError:
        raise ValueError(f'Unknown video format "{value}"') from None


def _frame_dtype(fmt: VideoFormat, sample_type, width: int, height: int) -> np.dtype:
    """One frame as a record of planes; odd luma sizes round the chroma up, as ffmpeg does."""
    w_div, h_div = _SUBSAMPLING[fmt]
    cw = (width + w_div - 1) // w_div if w_div else 0
    ch = (height + h_div - 1) // h_div if h_div else 0
    return np.dtype([("y", sample_type, (height, width)), ("u", sample_type, (ch, cw)), ("v", sample_type, (ch, cw))])


def get_raw_video_file_info(filename: str) -> Dict[str, Any]:
    """What the file name says: ``width``, ``height``, ``framerate`` (a Fraction), ``bitdepth``, ``format`` (a
    VideoFormat), ``endianness``, ``extension``; a field the name does not state is None.  {} if it says nothing.
    A name that states two different bit depths raises ValueError."""
    found: Dict[str, Any] = {}
    for pattern in _PATTERNS:
        m = re.search(pattern, filename)
        if m:
            found.update(m.groupdict())
    if not found:
        return {}
    info = {k: found.get(k) for k in ("width", "height", "framerate", "bitdepth", "format", "endianness", "extension")}
    depth2 = found.get("bitdepth2")
    if info["bitdepth"] and depth2 and info["bitdepth"] != depth2:
        raise ValueError(f'Filename "{filename}" specifies bit-depth twice.')
    if depth2:
        info["bitdepth"] = depth2
    if info["format"] is not None:
        info["format"] = _FORMAT_TAGS[info["format"].lower()]
    if info["endianness"] is not None:
        info["endianness"] = info["endianness"].lower()
    if info["framerate"] is not None:
        info["framerate"] = _NTSC_RATES.get(info["framerate"]) or Fraction(info["framerate"])
    for k in ("width", "height", "bitdepth"):
        if info[k] is not None:
            info[k] = int(info[k])
    return info


def _map_samples(filename, bitdepth: int) -> np.memmap:
    """The file as a read-only flat array of whole samples (a trailing odd byte of a 16-bit file is left out)."""
    sample = np.dtype(_SAMPLE_TYPES[bitdepth])
    return np.memmap(filename, dtype=sample, mode="r", shape=(os.path.getsize(filename) // sample.itemsize,))


class RawVideoSequence(Sequence):
    """A raw video file as a sequence of frames; ``seq[i]`` is a numpy record with fields ``y``, ``u``, ``v``.

    Args:
        mmap: the file as a flat array of samples
        width, height, bitdepth, format, framerate: the video's parameters
    """

    def __init__(self, mmap: np.ndarray, width: int, height: int, bitdepth: int, format: Union[VideoFormat, str],
                 framerate=None):
        if bitdepth not in _SAMPLE_TYPES:
            raise ValueError(f"Unsupported bit depth {bitdepth}")
        self.width, self.height, self.bitdepth, self.framerate = width, height, bitdepth, framerate
        self.format = _as_format(format)
        self.dtype = _frame_dtype(self.format, _SAMPLE_TYPES[bitdepth], width, height)
        nbytes = mmap.size * mmap.itemsize
        self.total_frms = nbytes // self.dtype.itemsize
        whole = self.total_frms * self.dtype.itemsize // mmap.itemsize
        self.data = mmap[:whole].view(self.dtype)     # a trailing partial frame is ignored

    @classmethod
    def new_like(cls, sequence: "RawVideoSequence", filename: str) -> "RawVideoSequence":
        mmap = _map_samples(filename, sequence.bitdepth)
        return cls(mmap, width=sequence.width, height=sequence.height, bitdepth=sequence.bitdepth,
                   format=sequence.format, framerate=sequence.framerate)

    @classmethod
    def from_file(cls, filename: str, width: Optional[int] = None, height: Optional[int] = None,
                  bitdepth: Optional[int] = None, format: Optional[VideoFormat] = None,
                  framerate=None) -> "RawVideoSequence":
        """Memory-map ``filename``; what is not given is read from the name.  RuntimeError if the size, the bit
        depth or the format stays unknown."""
        info = get_raw_video_file_info(os.path.basename(str(filename)))
        width = width or info.get("width")
        height = height or info.get("height")
        bitdepth = bitdepth or info.get("bitdepth")
        format = format or info.get("format")
        framerate = framerate or info.get("framerate")
        if width is None or height is None or bitdepth is None or format is None:
            raise RuntimeError(f"Could not get sequence information {filename}")
        if bitdepth not in _SAMPLE_TYPES:
            raise ValueError(f"Unsupported bit depth {bitdepth}")
        mmap = _map_samples(filename, bitdepth)
        return cls(mmap, width=width, height=height, bitdepth=bitdepth, format=format, framerate=framerate)

    def __getitem__(self, index: Union[int, slice]) -> Any:
        return self.data[index]

    def __len__(self) -> int:
        return len(self.data)

    def close(self):
        del self.data
