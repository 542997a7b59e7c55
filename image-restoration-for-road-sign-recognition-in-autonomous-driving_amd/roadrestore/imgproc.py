"""Device-batched image I/O around the networks.

The reference runs these per image on the host (cv2 / PIL / skimage in
DataLoader workers and in the inference loop).  Here they take a whole
[n, h, w, c] uint8 batch resident on the GPU and run as HIP kernels
(csrc/resize.hip, quality.hip, distort.hip) behind the C ABI:

* ``Resize`` / ``ToTensor`` / ``Normalize`` / ``Compose`` -- torchvision's
  transform names and argument meaning (17:66, 18:28-32); ``Resize`` is
  PIL's bilinear resample bit for bit, and ``Compose([Resize, ToTensor,
  Normalize])`` runs as one fused pass.
* ``apply_random_distortions`` -- 14:31-64, the per-image random draws made
  with Python's ``random`` in the reference's order, the noise field drawn on
  device (Philox4x32-10) instead of ``np.random.normal``.
* ``apply_compound_distortion`` -- 16:14-37 (blur 10 @ 45 deg, fog 0.5, noise
  var 0.02).
* ``cv_resize`` -- ``cv2.resize(img, (224, 224))`` of the 08 PSNR leg's
  clean image (08:118-119): OpenCV's INTER_LINEAR, which is not PIL's.
* ``psnr`` / ``ssim`` -- 08:123-125 (skimage semantics, data_range 255).
* ``restoration_quality`` -- the whole metric leg 08:118-125 for a batch:
  clean originals of unequal size (a ``RaggedBatch``; ``cv_resize`` and
  ``RaggedBatch.cv_resize`` take one too) against the restored batch, PSNR
  and SSIM in one fused call of two launches.
* ``RaggedBatch`` / ``read_ppm`` / ``ImageFolder`` / ``find_images`` -- the
  step before the first tensor: GTSRB's ``.ppm`` files have unequal sizes and
  the reference resizes each on its own (05:24-32, 14:68, 18:28-36).  A
  ``RaggedBatch`` holds n images of unequal size in one device buffer;
  ``Resize`` / ``Compose`` turn it into the dense batch in two launches.
* ``read_png`` / ``read_images`` -- the PNG files of 17:69-79, 18:35,
  07:52-66 and the mixed ``.ppm`` + ``.png`` list of 08:84-88 into the same
  ``RaggedBatch``: inflate on host threads, the row filters undone and
  ``convert('RGB')`` applied on the device for the whole batch in one launch.
* ``DynamicDistortionDataset`` -- 14:66-93: files -> ``(bad, clean)`` tensor
  pairs, the distortion applied to every image at its NATIVE size before the
  resize, as the reference does; ``apply_random_distortions``,
  ``apply_compound_distortion`` and ``RandomDistortion`` take a ``RaggedBatch``
  for that (two launches per batch, the blur input kept on chip).
* ``add_gaussian_noise`` / ``apply_motion_blur`` / ``add_fog`` -- the offline
  generators 02:12-27, 03:11-30 and 04:12-31 in THEIR arithmetic (fp64, the
  uint8 wrap of the noise, the per-image min-max stretch of the blur), which
  is not 14's; with ``low_clip=0`` / ``normalize=False`` / ``jitter=False``
  the three steps of 13:33-56.  ``SingleDistortionDataset`` makes the Noise,
  Blur or Fog pairs 07 trains on without the disk sets, ``PairedDataset`` is
  07:35-72 over sets that are on disk, ``write_ppm`` writes one.
"""
from __future__ import annotations

import ctypes as C
import os
import random as _random
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from . import ops
from ._lib import (PNG_REASON, RR_DISTORT_BLUR, RR_DISTORT_FOG, RR_DISTORT_KMAX, RR_DISTORT_NOISE,
                   RR_EUNSUPPORTED, RR_SINGLE_BLUR, RR_SINGLE_FOG, RR_SINGLE_NOISE, DistortParam, PngImage, PngInfo,
                   RaggedImage, SingleParam, lib)

__all__ = ["Resize", "ToTensor", "Normalize", "Compose", "apply_random_distortions",
           "encode_png", "write_png",
           "RandomDistortion", "motion_blur_table", "DynamicDistortionDataset",
           "apply_compound_distortion", "distortion_params", "psnr", "ssim", "cv_resize",
           "restoration_quality", "RaggedBatch", "read_ppm", "read_png", "read_images", "ImageFolder", "find_images",
           "add_gaussian_noise", "apply_motion_blur", "add_fog", "fog_transmissions", "SingleDistortionDataset",
           "PairedDataset", "write_ppm", "IMAGENET_MEAN", "IMAGENET_STD"]

IMAGENET_MEAN = (0.485, 0.456, 0.406)      # 18:31
IMAGENET_STD = (0.229, 0.224, 0.225)

# 14:23-25
PROB_NOISE = 0.5
PROB_BLUR = 0.5
PROB_FOG = 0.5


def _check_u8(x):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 4:
        raise TypeError("expected a [n, h, w, c] uint8 device batch")


class Resize:
    """torchvision ``Resize((h, w))`` on PIL images (bilinear): u8 -> u8."""

    def __init__(self, size):
        if isinstance(size, int):
            raise NotImplementedError("Resize(int) (aspect-preserving) is not used by the reference")
        self.size = (int(size[0]), int(size[1]))

    def __call__(self, x):
        if isinstance(x, RaggedBatch):
            return x.resize(self.size[0], self.size[1], out="u8")
        _check_u8(x)
        return ops.resize_bilinear_u8(x, self.size[0], self.size[1], out="u8")


class ToTensor:
    """u8 [n, h, w, c] -> fp32 [n, c, h, w] / 255."""

    def __call__(self, x):
        if isinstance(x, RaggedBatch):
            raise TypeError("ToTensor needs a dense batch: a RaggedBatch has no common shape "
                            "(put Resize first)")
        _check_u8(x)
        n, h, w, c = x.shape
        return ops.resize_bilinear_u8(x, h, w, out="f32")


class Normalize:
    """``(x - mean) / std`` per channel in fp32 (torchvision's
    ``sub_().div_()``).  It runs fused into the resample pass of
    ``Compose([Resize, ToTensor, Normalize])`` -- the only way the reference
    uses it (18:28-32); on its own it raises rather than fall back to ATen."""

    def __init__(self, mean, std):
        self.mean, self.std = tuple(mean), tuple(std)

    def __call__(self, x):
        raise NotImplementedError("Normalize runs fused: Compose([Resize(...), ToTensor(), "
                                  "Normalize(...)])")


class Compose:
    """Sequential transforms; ``[Resize, ToTensor]`` and ``[Resize, ToTensor,
    Normalize]`` prefixes fuse into one resample pass writing fp32 NCHW, for
    a dense batch and for a ``RaggedBatch`` alike."""

    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, x):
        t = self.transforms
        i = 0
        if len(t) >= 2 and isinstance(t[0], Resize) and isinstance(t[1], ToTensor):
            mean = std = None
            i = 2
            if len(t) >= 3 and isinstance(t[2], Normalize):
                mean, std = t[2].mean, t[2].std
                i = 3
            if isinstance(x, RaggedBatch):
                x = x.resize(t[0].size[0], t[0].size[1], out="f32", mean=mean, std=std)
            else:
                _check_u8(x)
                x = ops.resize_bilinear_u8(x, t[0].size[0], t[0].size[1], out="f32", mean=mean, std=std)
        for tr in t[i:]:
            x = tr(x)
        return x


# ---------------------------------------------------------------------------
# ragged batches: files of unequal size -> the first tensor

_RECORD = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4")])     # rr_ragged_image
assert _RECORD.itemsize == C.sizeof(RaggedImage) == 16


def _host_buffer(nbytes, device):
    """uint8 host staging buffer, pinned when it feeds a device copy"""
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8,
                       pin_memory=torch.device(device).type == "cuda")


class RaggedBatch:
    """n HWC uint8 images of unequal size in one buffer.

    ``data``: 1-D uint8 tensor; ``table``: [n, 16] uint8 tensor on the same
    device, n ``rr_ragged_image`` records (byte offset, h, w); ``sizes``: the
    host list of (h, w); ``channels``; ``max_hw``: the bound the device code
    holds every record to (the batch's own maximum unless given -- give it to
    keep one captured graph valid across batches).  ``records`` is a numpy
    array of the records or a sequence of (offset, h, w).

    The constructor runs ``rr_ragged_check`` on the host records against the
    buffer's size and raises ``ValueError`` if any image leaves it: nothing is
    launched.  ``Resize`` / ``Compose`` accept a RaggedBatch in place of the
    dense [n, h, w, c] tensor."""

    def __init__(self, data, records, channels=3, max_hw=None):
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1:
            raise TypeError("RaggedBatch data: expected a 1-D uint8 tensor")
        rec = np.ascontiguousarray(np.asarray(records, dtype=_RECORD).reshape(-1))
        n = rec.shape[0]
        if n == 0:
            raise ValueError("RaggedBatch: no images")
        if max_hw is None:
            max_hw = (max(int(rec["h"].max()), 1), max(int(rec["w"].max()), 1))
        max_hw = (int(max_hw[0]), int(max_hw[1]))
        rc = lib().rr_ragged_check(n, int(channels), data.numel(), rec.ctypes.data,
                                   max_hw[0], max_hw[1], max_hw[0], max_hw[1])
        if rc != 0:
            c = int(channels)
            bad = [i for i in range(n)
                   if not (1 <= rec["h"][i] <= max_hw[0] and 1 <= rec["w"][i] <= max_hw[1]
                           and 0 <= rec["offset"][i]
                           and int(rec["offset"][i]) + int(rec["h"][i]) * int(rec["w"][i]) * c <= data.numel())]
            where = f"image {bad[0]}: offset {int(rec['offset'][bad[0]])}, " \
                    f"{int(rec['h'][bad[0]])} x {int(rec['w'][bad[0]])}" if bad else f"channels {c}"
            raise ValueError(f"RaggedBatch: table rejected by rr_ragged_check ({rc}): {where}; "
                             f"buffer {data.numel()} bytes, bound {max_hw}")
        self.data = data.contiguous()
        self.records = rec
        self.channels = int(channels)
        self.max_hw = max_hw
        self.sizes = [(int(h), int(w)) for h, w in zip(rec["h"], rec["w"])]
        host = torch.from_numpy(rec.view(np.uint8).reshape(n, 16).copy())
        if data.is_cuda:
            host = host.pin_memory()
        self.table = host.to(data.device, non_blocking=True)

    def __len__(self):
        return len(self.sizes)

    @property
    def device(self):
        return self.data.device

    def to(self, device, non_blocking=False):
        """the batch on ``device``: one copy of the buffer, one of the table"""
        return RaggedBatch(self.data.to(device, non_blocking=non_blocking), self.records,
                           self.channels, self.max_hw)

    @classmethod
    def from_arrays(cls, images, device):
        """A list of [h, w, c] (or [h, w]) uint8 numpy arrays / torch tensors
        of unequal sizes -> RaggedBatch on ``device``: the images are packed
        back to back into one host buffer and copied in one H2D copy."""
        arrs = []
        for im in images:
            a = im.detach().cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
            if a.dtype != np.uint8 or a.ndim not in (2, 3):
                raise TypeError("RaggedBatch.from_arrays: expected [h, w, c] uint8 images")
            arrs.append(a[:, :, None] if a.ndim == 2 else a)
        if not arrs:
            raise ValueError("RaggedBatch: no images")
        c = arrs[0].shape[2]
        if any(a.shape[2] != c for a in arrs):
            raise ValueError("RaggedBatch.from_arrays: images differ in channel count")
        rec = np.zeros(len(arrs), dtype=_RECORD)
        rec["h"] = [a.shape[0] for a in arrs]
        rec["w"] = [a.shape[1] for a in arrs]
        nbytes = np.array([a.size for a in arrs], dtype=np.int64)
        rec["offset"] = np.cumsum(nbytes) - nbytes
        host = _host_buffer(nbytes.sum(), device)
        buf = host.numpy()
        for a, o, nb in zip(arrs, rec["offset"], nbytes):
            buf[o:o + nb] = a.reshape(-1)
        return cls(host[:max(int(nbytes.sum()), 1)].to(device, non_blocking=True), rec, c)

    def with_data(self, data):
        """another buffer under this batch's records: the batch an op returns
        that writes every image at its own offset (the ragged distortions).
        It SHARES ``table``, ``records`` and ``max_hw`` -- no check, no copy,
        nothing a graph capture could not hold -- so a table overwritten in
        place is seen through both."""
        if (not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1
                or data.numel() != self.data.numel() or data.device != self.data.device
                or not data.is_contiguous()):
            raise TypeError("RaggedBatch.with_data: expected a contiguous 1-D uint8 buffer of the same "
                            "size on the same device")
        b = object.__new__(RaggedBatch)
        b.data, b.records, b.channels, b.max_hw = data, self.records, self.channels, self.max_hw
        b.sizes, b.table = self.sizes, self.table
        return b

    def resize(self, oh, ow, out="u8", mean=None, std=None):
        """every image through PIL's bilinear resample to (oh, ow): the dense
        [n, oh, ow, c] uint8 or [n, c, oh, ow] fp32 batch (ops.resize_ragged_u8)"""
        if mean is not None and (len(mean) != self.channels or len(std) != self.channels):
            raise ValueError(f"Normalize: {len(mean)} means for {self.channels} channels")
        return ops.resize_ragged_u8(self.data, self.table, self.max_hw, self.channels, oh, ow,
                                    out=out, mean=mean, std=std)

    def cv_resize(self, size):
        """every image through ``cv2.resize(img, (w, h))`` (INTER_LINEAR,
        08:118-119), ``size`` = (w, h) in cv2's order: the dense [n, h, w, c]
        uint8 batch, in one launch (ops.cv_resize_ragged_u8)"""
        ow, oh = size
        return ops.cv_resize_ragged_u8(self.data, self.table, self.max_hw, self.channels, oh, ow)


_PPM_WS = b" \t\n\r\x0b\x0c"
_PPM_HEAD = 1 << 16            # a header (comments included) is searched this far


def _ppm_header(head, path):
    """The first bytes of a binary PPM -> (w, h, maxval, payload offset).
    Netpbm's grammar: the magic "P6", then width, height and maxval in decimal,
    separated by any whitespace, with "#" comments running to the end of their
    line; exactly ONE whitespace byte after maxval, and the pixels follow (they
    may themselves look like whitespace or digits)."""
    if head[:2] != b"P6":
        raise ValueError(f"{path}: not a binary PPM (magic {bytes(head[:2])!r}, expected b'P6')")
    n, pos, vals = len(head), 2, []
    if n < 3 or not (head[2] in _PPM_WS or head[2] == 0x23):
        raise ValueError(f"{path}: malformed PPM header")
    for _ in range(3):
        while pos < n and (head[pos] in _PPM_WS or head[pos] == 0x23):
            if head[pos] == 0x23:
                while pos < n and head[pos] not in b"\r\n":
                    pos += 1
            else:
                pos += 1
        start = pos
        while pos < n and 0x30 <= head[pos] <= 0x39:
            pos += 1
        if pos == start:
            raise ValueError(f"{path}: malformed PPM header")
        vals.append(int(head[start:pos]))
    if pos >= n or head[pos] not in _PPM_WS:
        raise ValueError(f"{path}: malformed PPM header (no whitespace after maxval)")
    return vals[0], vals[1], vals[2], pos + 1


def _read_ppm_file(path, buf, a, b):
    """one binary PPM file into buf[a:b] -> (byte offset of the pixels in the file, h, w);
    ValueError naming the file unless it is an 8-bit P6 with all its pixels"""
    with open(path, "rb") as f:
        got = f.readinto(memoryview(buf[a:b])) if b > a else 0
    w, h, maxval, off = _ppm_header(bytes(buf[a:a + min(got, _PPM_HEAD)]), path)
    if not 1 <= maxval <= 255:
        raise ValueError(f"{path}: maxval {maxval}: only 8-bit PPM (maxval <= 255) is read")
    if h < 1 or w < 1 or h > 2 ** 31 - 1 or w > 2 ** 31 - 1:
        raise ValueError(f"{path}: bad PPM size {w} x {h}")
    if off + h * w * 3 > got:
        raise ValueError(f"{path}: truncated PPM: {w} x {h} needs {h * w * 3} pixel bytes, "
                         f"{max(got - off, 0)} present")
    return off, h, w


def read_ppm(paths, device, threads=0):
    """Binary PPM files (P6, maxval <= 255: what GTSRB ships) -> RaggedBatch on
    ``device``.  The whole files are read by a thread pool into one host
    buffer (pinned for a GPU), their headers parsed on the host, and the table
    offsets point just past each header: the decode IS the offset.  One
    non-blocking H2D copy moves all of it.  ``threads``: pool size, 0 = up to
    8.  Any other file (P3, P5, 16-bit, truncated) raises ``ValueError`` naming
    it.  Samples are taken as stored (GTSRB's maxval is 255; a smaller maxval
    is not rescaled).  With ``device="cpu"`` the batch stays on the host
    (``.to(device)`` later)."""
    paths = [os.fspath(p) for p in paths]
    n = len(paths)
    if n == 0:
        raise ValueError("read_ppm: no paths")
    fsize = np.array([os.path.getsize(p) for p in paths], dtype=np.int64)
    start = np.cumsum(fsize) - fsize
    total = int(fsize.sum())
    host = _host_buffer(total, device)
    buf = host.numpy()
    rec = np.zeros(n, dtype=_RECORD)

    def one(i):
        a = int(start[i])
        off, h, w = _read_ppm_file(paths[i], buf, a, a + int(fsize[i]))
        rec[i] = (a + off, h, w)

    workers = int(threads) if threads else min(8, n)
    if workers <= 1:
        for i in range(n):
            one(i)
    else:
        with ThreadPoolExecutor(workers) as pool:
            list(pool.map(one, range(n)))
    return RaggedBatch(host[:max(total, 1)].to(device, non_blocking=True), rec, 3)


# ---------------------------------------------------------------------------
# PNG input (17:69-79, 18:35, 07:52-66, 08:84-88): host inflate, device unfilter

_PNG_RECORD = np.dtype([("src", "<i8"), ("dst", "<i8"), ("h", "<i4"), ("w", "<i4"),
                        ("channels", "<i4"), ("kind", "<i4")])                  # rr_png_image
_PNG_INFO = np.dtype([("h", "<i4"), ("w", "<i4"), ("channels", "<i4"), ("status", "<i4"),
                      ("reason", "<i4")])                                       # rr_png_info
assert _PNG_RECORD.itemsize == C.sizeof(PngImage) == 32
assert _PNG_INFO.itemsize == C.sizeof(PngInfo) == 20


def _png_raise(paths, info):
    """ValueError naming the first file rr_png_probe / rr_png_inflate refused"""
    for p, st, why in zip(paths, info["status"], info["reason"]):
        if st != 0:
            raise ValueError(f"{p}: {PNG_REASON.get(int(why), f'reason {int(why)}')} "
                             f"({'unsupported' if st == RR_EUNSUPPORTED else 'invalid'} PNG)")


def _stage_files(paths, is_png, device, threads):
    """The host half of ``_read_files``: probe, one host buffer (PNG: the
    inflated scanlines, PPM: the file) with the rr_png_image table behind it
    at a 16-byte boundary -> (host buffer, records, data bytes, table offset,
    output bytes, (max_h, max_w)).  Raises ValueError for a bad file."""
    n = len(paths)
    L = lib()
    workers = int(threads) if threads else min(8, n)
    rec = np.zeros(n, dtype=_PNG_RECORD)
    png = [i for i in range(n) if is_png[i]]
    ppm = [i for i in range(n) if not is_png[i]]
    slot = np.zeros(n, dtype=np.int64)
    if png:
        sub = (C.c_char_p * len(png))(*[os.fsencode(paths[i]) for i in png])
        info = np.zeros(len(png), dtype=_PNG_INFO)
        L.rr_png_probe(len(png), C.cast(sub, C.c_void_p), info.ctypes.data, workers)
        _png_raise([paths[i] for i in png], info)
        rec["h"][png], rec["w"][png], rec["channels"][png] = info["h"], info["w"], info["channels"]
        rec["kind"][png] = 1
        slot[png] = info["h"].astype(np.int64) * (1 + info["w"].astype(np.int64) * info["channels"])
    for i in ppm:
        slot[i] = os.path.getsize(paths[i])
        rec["channels"][i] = 3
    start = np.cumsum(slot) - slot
    data_bytes = int(slot.sum())
    table_off = (data_bytes + 15) & ~15
    host = _host_buffer(table_off + 32 * n, device)
    buf = host.numpy()
    rec["src"] = start

    def one_ppm(i):
        a = int(start[i])
        off, h, w = _read_ppm_file(paths[i], buf, a, a + int(slot[i]))
        rec[i] = (a + off, 0, h, w, 3, 0)

    if workers <= 1 or len(ppm) <= 1:
        for i in ppm:
            one_ppm(i)
    else:
        with ThreadPoolExecutor(workers) as pool:
            list(pool.map(one_ppm, ppm))
    if png:
        arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
        info = np.zeros(n, dtype=_PNG_INFO)
        L.rr_png_inflate(n, C.cast(arr, C.c_void_p), rec.ctypes.data, host.data_ptr(), data_bytes,
                         info.ctypes.data, workers)
        _png_raise(paths, info)
    nb = rec["h"].astype(np.int64) * rec["w"] * 3
    rec["dst"] = np.cumsum(nb) - nb
    out_bytes = int(nb.sum())
    max_hw = (int(rec["h"].max()), int(rec["w"].max()))
    rc = L.rr_png_table_check(n, data_bytes, out_bytes, rec.ctypes.data, max_hw[0], max_hw[1])
    if rc != 0:
        raise ValueError(f"read_png: table rejected by rr_png_table_check ({rc}): sizes up to {max_hw}"
                         + (" (widths above 8192 are not read)" if rc == RR_EUNSUPPORTED else ""))
    buf[table_off:table_off + 32 * n] = rec.view(np.uint8)
    return host, rec, data_bytes, table_off, out_bytes, max_hw


def _read_files(paths, is_png, device, threads):
    """PNG and binary-PPM files, in the order of ``paths``, -> RaggedBatch of
    RGB images on ``device``: the host stage, one H2D copy of buffer and
    table, one launch (ops.png_unfilter)."""
    n = len(paths)
    host, rec, data_bytes, table_off, out_bytes, max_hw = _stage_files(paths, is_png, device, threads)
    dev = host.to(device, non_blocking=True)
    out = ops.png_unfilter(dev[:data_bytes], dev[table_off:table_off + 32 * n].view(n, 32), max_hw,
                           out_bytes)
    images = np.zeros(n, dtype=_RECORD)
    images["offset"], images["h"], images["w"] = rec["dst"], rec["h"], rec["w"]
    return RaggedBatch(out, images, 3)


def read_png(paths, device, threads=0):
    """PNG files (8-bit grey, grey + alpha, RGB or RGBA, no interlace: what
    cv2.imwrite / PIL save and imgproc.write_png writes) -> RaggedBatch of RGB
    images on ``device``, each as ``Image.open(p).convert('RGB')`` gives it
    (17:69-79, 18:35, 07:52-66): grey replicated, alpha dropped.  The host
    probes the headers, inflates every file's IDAT stream on ``threads``
    threads (0 = up to 8) into one pinned buffer and copies it with the record
    table in one non-blocking H2D copy; the row filters are undone on the
    device for the whole batch in one launch.  A file that is not such a PNG
    (palette, 16-bit, interlaced, bad CRC, truncated, wrong inflated size, bad
    filter byte) raises ``ValueError`` naming it and the reason before
    anything is launched.  No CPU path: ``device="cpu"`` raises."""
    paths = [os.fspath(p) for p in paths]
    if not paths:
        raise ValueError("read_png: no paths")
    return _read_files(paths, [True] * len(paths), device, threads)


def read_images(paths, device, threads=0):
    """Image files by extension -> one RaggedBatch in the order of ``paths``:
    all ``.ppm`` -> ``read_ppm`` (unchanged, zero-copy); all ``.png`` ->
    ``read_png``; a mixed list (08:84-88) -> one buffer, one table of PNG and
    raw records, one launch."""
    paths = [os.fspath(p) for p in paths]
    if not paths:
        raise ValueError("read_images: no paths")
    ext = [os.path.splitext(p)[1].lower() for p in paths]
    for p, e in zip(paths, ext):
        if e not in (".ppm", ".png"):
            raise ValueError(f"{p}: only .ppm and .png files are read")
    if all(e == ".ppm" for e in ext):
        return read_ppm(paths, device, threads)
    return _read_files(paths, [e == ".png" for e in ext], device, threads)


def find_images(root, pattern="*/*.ppm"):
    """``sorted(Path(root).glob(pattern))``: the file list of 14:68"""
    return sorted(Path(root).glob(pattern))


class ImageFolder:
    """torchvision ``ImageFolder``'s view of a directory tree (05:32, 18:35),
    read straight into device batches.  ``classes``: the sorted sub-directory
    names of ``root``; ``class_to_idx``; ``samples``: (path, class index) in
    class order and, within a class, in ``sorted(os.walk(dir))`` order with
    each directory's file names sorted; the extension match ignores case.  A
    class without files keeps its index (torchvision's ``find_classes`` counts
    it too) and contributes no samples.  ``extensions``: ``(".ppm",)`` by
    default; ``(".png",)`` or ``(".ppm", ".png")`` list PNG files too (18:35
    over the directory 17:89-99 wrote) and load them through ``read_images``.

    ``load(indices, device)`` -> (RaggedBatch, int64 labels on ``device``);
    ``batches(batch_size, shuffle, generator)`` yields that for one pass over
    the samples, the last batch short (``DataLoader(drop_last=False)``).
    ``device`` defaults to the GPU when there is one."""

    def __init__(self, root, extensions=(".ppm",), device=None, threads=0):
        self.root = os.fspath(root)
        self.extensions = tuple(e.lower() for e in extensions)
        self.device = torch.device(device if device is not None
                                   else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.threads = threads
        self.classes = sorted(e.name for e in os.scandir(self.root) if e.is_dir())
        if not self.classes:
            raise FileNotFoundError(f"Couldn't find any class folder in {self.root}.")
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.samples = []
        for c in self.classes:
            for d, _, names in sorted(os.walk(os.path.join(self.root, c), followlinks=True)):
                for name in sorted(names):
                    if name.lower().endswith(self.extensions):
                        self.samples.append((os.path.join(d, name), self.class_to_idx[c]))
        self.targets = [t for _, t in self.samples]

    def __len__(self):
        return len(self.samples)

    def load(self, indices, device=None):
        device = self.device if device is None else torch.device(device)
        indices = [int(i) for i in indices]
        batch = read_images([self.samples[i][0] for i in indices], device, self.threads)
        labels = torch.tensor([self.samples[i][1] for i in indices], dtype=torch.int64)
        if device.type == "cuda":
            labels = labels.pin_memory()
        return batch, labels.to(device, non_blocking=True)

    def batches(self, batch_size, shuffle=False, generator=None, device=None):
        n = len(self.samples)
        order = torch.randperm(n, generator=generator).tolist() if shuffle else list(range(n))
        for a in range(0, n, int(batch_size)):
            yield self.load(order[a:a + int(batch_size)], device)


def distortion_params(n, rng=None):
    """Per-image draws of apply_random_distortions (14:36-58) in the
    reference's order with Python's ``random``: -> (params, taps [n, K, K])."""
    rng = rng or _random
    params, taps = [], torch.zeros(n, RR_DISTORT_KMAX, RR_DISTORT_KMAX)
    for i in range(n):
        p = DistortParam(0.0, 1.0, 0.0, 0, 0)
        if rng.random() < PROB_FOG:
            intensity = rng.uniform(0.3, 0.7)
            A = 0.9
            t = 1.0 - intensity * rng.uniform(0.8, 1.2)
            p.flags |= RR_DISTORT_FOG
            p.fog_mul, p.fog_add = t, A * (1 - t)          # stored as fp32, as numpy casts them
        if rng.random() < PROB_NOISE:
            var = rng.uniform(0.01, 0.03)
            p.flags |= RR_DISTORT_NOISE
            p.sigma = var ** 0.5
        if rng.random() < PROB_BLUR:
            degree = rng.randint(5, 15)
            angle = rng.randint(0, 360)
            if degree > 1:
                p.flags |= RR_DISTORT_BLUR
                p.ksize = degree
                taps[i] = ops.motion_blur_kernel(degree, angle)
        params.append(p)
    return params, taps


def _distort_ragged(x, params, taps, mode, noise, seed):
    """ops.distort_ragged_u8 on a RaggedBatch -> the RaggedBatch of the results
    under the same records (``noise``: 1-D fp64, packed in table order)"""
    ops._need_cuda(x.data)
    if noise is not None:
        noise = noise.reshape(-1)
    y = ops.distort_ragged_u8(x.data, x.table, x.max_hw, x.channels, params, taps, mode=mode,
                              noise=noise, seed=seed)
    return x.with_data(y)


def apply_random_distortions(x, rng=None, seed=None, noise=None):
    """14:31-64 on a [n, h, w, c] uint8 device batch, or on a RaggedBatch:
    every image at its native size, as 14:75-93 calls it before the resize
    (-> a RaggedBatch under the same records)."""
    ragged = isinstance(x, RaggedBatch)
    if not ragged:
        _check_u8(x)
    params, taps = distortion_params(len(x) if ragged else x.shape[0], rng)
    if seed is None:
        seed = (rng or _random).getrandbits(64)
    if ragged:
        return _distort_ragged(x, params, taps, 0, noise, seed)
    return ops.distort_u8(x, params, taps, mode=0, noise=noise, seed=seed)


_TABLES = {}


def motion_blur_table(device):
    """Device copy of every motion-blur kernel the draws can pick (degree
    5..15 x angle 0..360, [11, 361, KMAX, KMAX] fp32), built once on the host
    by the same restatement of cv2 getRotationMatrix2D + warpAffine."""
    key = str(device)
    t = _TABLES.get(key)
    if t is None:
        L = ops.lib()
        nf = L.rr_motion_blur_table_floats()
        host = torch.empty(nf, dtype=torch.float32)
        L.check(L.rr_motion_blur_table(C.c_void_p(host.data_ptr())), "rr_motion_blur_table")
        t = _TABLES[key] = host.view(11, 361, RR_DISTORT_KMAX, RR_DISTORT_KMAX).to(device)
    return t


class RandomDistortion:
    """apply_random_distortions (14:31-64) for a whole [n, h, w, c] uint8
    device batch with the per-image draws made ON DEVICE
    (rr_distort_random_u8): graph-capturable, so a captured training step
    re-draws on every replay.  The draws follow the reference's distributions
    (Philox4x32-10 keyed by (seed, step); the reference's stream is unseeded);
    the step counter lives in device memory and advances once per call.  A
    ``RaggedBatch`` in place of the tensor is distorted image by image at
    native size and comes back as a ``RaggedBatch`` under the same records.

    ``last_draws()`` reads the most recent draws back (tests)."""

    def __init__(self, device, seed=0):
        self.device = torch.device(device)
        self.seed = int(seed) & (2 ** 64 - 1)
        self.step = torch.zeros((), dtype=torch.int64, device=self.device)
        self.table = motion_blur_table(self.device)
        self._ws = None
        self._shape = None

    def __call__(self, x, out=None):
        if isinstance(x, RaggedBatch):
            return self._ragged(x, out)
        _check_u8(x)
        ops._need_cuda(x)
        n, h, w, c = x.shape
        if self._ws is None or self._shape != (n, h, w, c):
            self._ws = ops._ws(lib().rr_distort_random_workspace(n, h, w, c), self.device)
            self._shape = (n, h, w, c)
        return ops.distort_random_u8(x, self.seed, self.step, self.table, self._ws, out)

    def _ragged(self, x, out):
        """a RaggedBatch: every image at its native size, as 14:75-93 distorts
        the file's pixels before the resize (rr_distort_random_ragged_u8) ->
        the RaggedBatch of the results under the same records.  Image i draws
        what image i of a dense batch draws at the same (seed, step)."""
        ops._need_cuda(x.data, x.table)
        n, c, (max_h, max_w) = len(x), x.channels, x.max_hw
        shape = ("ragged", n, c, max_h, max_w)
        if self._ws is None or self._shape != shape:
            self._ws = ops._ws(lib().rr_distort_ragged_workspace(n, c, max_h, max_w), self.device)
            self._shape = shape
        if out is None:
            out = torch.empty_like(x.data)
        y = x.with_data(out)                            # checks out against the batch's buffer
        ops.distort_random_ragged_u8(x.data, x.table, x.max_hw, c, self.seed, self.step, self.table,
                                     self._ws, out)
        return y

    def last_draws(self):
        """-> (params: list of DistortParam, table index [n] int32, noise seed)"""
        po, io, so = C.c_size_t(), C.c_size_t(), C.c_size_t()
        ragged = self._shape[0] == "ragged"
        dims = self._shape[1:] if ragged else self._shape          # (n, c, max_h, max_w) or (n, h, w, c)
        name = "rr_distort_random_ragged_draws" if ragged else "rr_distort_random_draws"
        lib().check(getattr(lib(), name)(*dims, self._ws.data_ptr(), C.byref(po), C.byref(io), C.byref(so)), name)
        n = dims[0]
        raw = self._ws.cpu()
        sz = C.sizeof(DistortParam)
        arr = (DistortParam * n).from_buffer_copy(bytes(raw[po.value:po.value + n * sz].numpy()))
        idx = raw[io.value:io.value + 4 * n].view(torch.int32).clone()
        seed = int(raw[so.value:so.value + 8].view(torch.int64).item()) & (2 ** 64 - 1)
        return list(arr), idx, seed


def apply_compound_distortion(x, seed=0, noise=None):
    """16:14-37 on a [n, h, w, c] uint8 device batch: blur (10, 45 deg) ->
    fog (intensity 0.5, A 0.9) -> noise (var 0.02); or on a RaggedBatch, every
    image at its native size as the offline generator reads it (16:44-58) ->
    a RaggedBatch under the same records."""
    ragged = isinstance(x, RaggedBatch)
    if not ragged:
        _check_u8(x)
    n = len(x) if ragged else x.shape[0]
    t, A = 1.0 - 0.5, 0.9
    p = DistortParam(0.02 ** 0.5, t, A * (1 - t), RR_DISTORT_FOG | RR_DISTORT_NOISE | RR_DISTORT_BLUR, 10)
    taps = ops.motion_blur_kernel(10, 45).unsqueeze(0).expand(n, -1, -1).contiguous()
    if ragged:
        return _distort_ragged(x, [p] * n, taps, 1, noise, seed)
    return ops.distort_u8(x, [p] * n, taps, mode=1, noise=noise, seed=seed)


class DynamicDistortionDataset:
    """The reference's training dataset (14:66-93) in device batches: the file
    list is ``sorted(clean_root.glob('*/*.ppm'))`` (14:68) and ``len()`` its
    length (14:72-73).  ``load(indices)`` reads those files with ONE
    ``read_ppm`` into a RaggedBatch (the clean images), distorts that batch at
    native size with an owned ``RandomDistortion(device, seed)`` (14:83: the
    draws on device, one step per batch), and puts both through ``transform``
    (14:86-91) -> ``(bad, clean)``, 14:93's order.  With 14:202-205's
    ``Compose([Resize((224, 224)), ToTensor()])`` these are two [n, 3, 224, 224]
    fp32 tensors; without a transform, two RaggedBatch.  ``batches(batch_size,
    shuffle, generator)`` yields that for one pass over the files, the last
    batch short.  The constructor lists files only and touches no device;
    ``device`` defaults to the GPU when there is one.  ``last_draws()``: the
    draws of the most recent batch."""

    def __init__(self, clean_root, transform=None, device=None, seed=0, threads=0):
        self.clean_files = sorted(Path(clean_root).glob('*/*.ppm'))
        self.transform = transform
        self.device = device
        self.seed = seed
        self.threads = threads
        self._distort = None

    def __len__(self):
        return len(self.clean_files)

    def _device(self):
        return torch.device(self.device if self.device is not None
                            else ("cuda" if torch.cuda.is_available() else "cpu"))

    def load(self, indices):
        if self._distort is None:
            self._distort = RandomDistortion(self._device(), self.seed)
        clean = read_ppm([self.clean_files[int(i)] for i in indices], self._distort.device, self.threads)
        bad = self._distort(clean)
        if self.transform is not None:
            bad, clean = self.transform(bad), self.transform(clean)
        return bad, clean

    def batches(self, batch_size, shuffle=False, generator=None):
        n = len(self.clean_files)
        order = torch.randperm(n, generator=generator).tolist() if shuffle else list(range(n))
        for a in range(0, n, int(batch_size)):
            yield self.load(order[a:a + int(batch_size)])

    def last_draws(self):
        return self._distort.last_draws()


# ---------------------------------------------------------------------------
# the single distortions of the offline generators 02-04 (the sets 07's three
# SimpleUNet restorers train on) and of 13:33-56, in their own arithmetic

def _as_ragged(x):
    """a [n, h, w, c] uint8 device tensor as the RaggedBatch of n equal images
    over the same bytes (no dense kernels: a uniform table) -> (batch, shape or
    None for a RaggedBatch)"""
    if isinstance(x, RaggedBatch):
        ops._need_cuda(x.data)
        return x, None
    _check_u8(x)
    ops._need_cuda(x)
    n, h, w, c = x.shape
    if n * h * w * c == 0:
        raise ValueError(f"empty batch {tuple(x.shape)}")
    rec = np.zeros(n, dtype=_RECORD)
    rec["offset"] = np.arange(n, dtype=np.int64) * (h * w * c)
    rec["h"], rec["w"] = h, w
    return RaggedBatch(x.contiguous().view(-1), rec, c), tuple(x.shape)


def _single(x, kind, params, taps=None, noise=None, seed=0):
    b, shape = _as_ragged(x)
    if noise is not None:
        noise = noise.reshape(-1)
    y = ops.distort_single_ragged_u8(b.data, b.table, b.max_hw, b.channels, kind, params, taps=taps,
                                     noise=noise, seed=seed)
    return b.with_data(y) if shape is None else y.view(shape)


def add_gaussian_noise(x, var=0.01, low_clip=-1.0, seed=None, noise=None):
    """02_gen_noise.py:12-27 on a [n, h, w, c] uint8 device batch or a
    RaggedBatch (-> the same kind): ``clip(image / 255 + N(0, var), low_clip,
    1) * 255`` in fp64, then ``np.uint8``, which truncates toward zero and
    wraps the negatives modulo 256 -- the Noise set carries that.
    ``low_clip=-1.0`` is 02:21-25 for every image (its branch is inert when no
    element is negative); ``low_clip=0.0`` is 13:33-38.  The field is drawn on
    the device (Philox4x32-10 keyed by ``seed``, drawn from ``random`` when
    None, and the packed element index) unless ``noise`` gives it: fp64, the
    reference's ``np.random.normal(0, var ** 0.5, shape)``, in packed element
    order."""
    n = len(x) if isinstance(x, RaggedBatch) else x.shape[0]
    if seed is None:
        seed = _random.getrandbits(64)
    p = SingleParam(float(var) ** 0.5, float(low_clip), 0, 0)
    return _single(x, RR_SINGLE_NOISE, [p] * n, noise=noise, seed=seed)


def apply_motion_blur(x, degree=10, angle=45, normalize=True):
    """03_gen_blur.py:11-30: ``cv2.filter2D`` with the rotated line kernel,
    then ``cv2.normalize(blurred, blurred, 0, 255, NORM_MINMAX)`` (03:29),
    which stretches every image's own range, taken over all channels, to
    0..255 -- a flat image comes out black.  ``normalize=False`` is 13:40-48.
    ``degree`` is the kernel's side, at most RR_DISTORT_KMAX."""
    n = len(x) if isinstance(x, RaggedBatch) else x.shape[0]
    taps = ops.motion_blur_kernel(degree, angle).unsqueeze(0).expand(n, -1, -1).contiguous()
    p = SingleParam(0.0, 0.0, int(degree), 1 if normalize else 0)
    return _single(x, RR_SINGLE_BLUR, [p] * n, taps=taps)


def fog_transmissions(n, fog_intensity=0.8, rng=None, jitter=True):
    """the n values of t that add_fog uses: 04:24-25, one ``rng.uniform(0.8,
    1.2)`` per image in batch order and the clip to [0.1, 0.9]; without
    ``jitter`` 13:54's ``1 - fog_intensity``, unclipped"""
    rng = rng or _random
    if not jitter:
        return [1.0 - fog_intensity] * n
    return [min(max(1.0 - fog_intensity * rng.uniform(0.8, 1.2), 0.1), 0.9) for _ in range(n)]


def add_fog(x, fog_intensity=0.8, rng=None, jitter=True):
    """04_gen_fog.py:12-31: ``clip((image / 255 * t + A (1 - t)) * 255, 0,
    255)`` truncated, in fp64, A = 0.9, t drawn per image as 04:24-25 draws it
    (``fog_transmissions``: Python's ``random``, or ``rng``);
    ``jitter=False`` is 13:50-56's fixed t."""
    n = len(x) if isinstance(x, RaggedBatch) else x.shape[0]
    A = 0.9
    params = [SingleParam(t, A * (1 - t), 0, 0) for t in fog_transmissions(n, fog_intensity, rng, jitter)]
    return _single(x, RR_SINGLE_FOG, params)


def _device_or_default(device):
    return torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))


def _batches(n, batch_size, shuffle, generator, load):
    order = torch.randperm(n, generator=generator).tolist() if shuffle else list(range(n))
    for a in range(0, n, int(batch_size)):
        yield load(order[a:a + int(batch_size)])


class SingleDistortionDataset:
    """What 02 / 03 / 04 write to disk and 07 reads back, made on the device
    instead: ``task`` is 'Noise' (02:44: var 0.02), 'Blur' (03:41: degree 12,
    angle 45, with the stretch) or 'Fog' (04:42: intensity 0.8).  The file
    list is DynamicDistortionDataset's (``sorted(clean_root.glob('*/*.ppm'))``);
    ``load(indices)`` reads the files with one ``read_ppm``, distorts the
    batch at native size and puts both through ``transform`` -> ``(bad,
    clean)``, 07:72's order; ``batches(batch_size, shuffle, generator)``
    yields that for one pass, the last batch short.  The noise seeds and the
    fog draws come from an owned ``random.Random(seed)``.  The constructor
    lists files only and touches no device."""

    TASKS = ("Noise", "Blur", "Fog")

    def __init__(self, clean_root, task, transform=None, device=None, seed=0, threads=0):
        if task not in self.TASKS:
            raise ValueError(f"task {task!r}: one of {self.TASKS}")
        self.clean_files = sorted(Path(clean_root).glob('*/*.ppm'))
        self.task = task
        self.transform = transform
        self.device = device
        self.threads = threads
        self.rng = _random.Random(seed)

    def __len__(self):
        return len(self.clean_files)

    def distort(self, clean):
        if self.task == "Noise":
            return add_gaussian_noise(clean, var=0.02, seed=self.rng.getrandbits(64))
        if self.task == "Blur":
            return apply_motion_blur(clean, degree=12, angle=45)
        return add_fog(clean, fog_intensity=0.8, rng=self.rng)

    def load(self, indices):
        clean = read_ppm([self.clean_files[int(i)] for i in indices], _device_or_default(self.device),
                         self.threads)
        bad = self.distort(clean)
        if self.transform is not None:
            bad, clean = self.transform(bad), self.transform(clean)
        return bad, clean

    def batches(self, batch_size, shuffle=False, generator=None):
        return _batches(len(self.clean_files), batch_size, shuffle, generator, self.load)


class PairedDataset:
    """07_train_restoration.py:35-72 from disk, in device batches.
    ``data_pairs`` is built as 07:42-55 builds it: the clean files are
    ``sorted(clean_root.glob('*/*.ppm'))``, the distorted file has the same
    relative path under ``distorted_root``, with the suffix ``.png`` only if
    that does not exist, and a clean file without either is dropped.
    ``load(indices)`` reads both sides with ``read_images`` and puts them
    through ``transform`` -> ``(bad, clean)`` (07:72); ``batches`` as
    SingleDistortionDataset's.  The constructor touches no device."""

    def __init__(self, clean_root, distorted_root, transform=None, device=None, threads=0):
        self.clean_root = Path(clean_root)
        self.distorted_root = Path(distorted_root)
        self.transform = transform
        self.device = device
        self.threads = threads
        self.clean_files = sorted(self.clean_root.glob('*/*.ppm'))
        self.data_pairs = []
        for c_path in self.clean_files:
            d_path = self.distorted_root / c_path.relative_to(self.clean_root)
            if not d_path.exists():
                d_path = d_path.with_suffix('.png')
            if d_path.exists():
                self.data_pairs.append((d_path, c_path))

    def __len__(self):
        return len(self.data_pairs)

    def load(self, indices):
        device = _device_or_default(self.device)
        pairs = [self.data_pairs[int(i)] for i in indices]
        bad = read_images([d for d, _ in pairs], device, self.threads)
        clean = read_images([c for _, c in pairs], device, self.threads)
        if self.transform is not None:
            bad, clean = self.transform(bad), self.transform(clean)
        return bad, clean

    def batches(self, batch_size, shuffle=False, generator=None):
        return _batches(len(self.data_pairs), batch_size, shuffle, generator, self.load)


def write_ppm(images, paths, threads=0):
    """Binary PPM writer (P6, maxval 255: the header ``cv2.imwrite`` writes to
    a ``.ppm`` path, so a set lands where 02:54, 03:46 and 04:47 write it) for
    an [n, h, w, 3] uint8 batch or a 3-channel RaggedBatch, device or host.
    One D2H copy of the whole buffer, then ``threads`` host threads (0 = up to
    8) write the files; parent directories are created.  ``read_ppm`` reads
    the files back byte for byte.  The bytes are written as they lie: the
    files hold the batch's channel order."""
    paths = [os.fspath(p) for p in paths]
    if isinstance(images, RaggedBatch):
        if images.channels != 3:
            raise ValueError(f"write_ppm: {images.channels} channels (a PPM holds 3)")
        host = images.data.cpu().numpy()
        recs = [(int(o), int(h), int(w)) for o, h, w in images.records]
    else:
        if (not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4
                or images.shape[-1] != 3):
            raise ValueError("write_ppm: expected an [n, h, w, 3] uint8 tensor or a RaggedBatch")
        n, h, w, _ = images.shape
        host = images.contiguous().cpu().numpy().reshape(-1)
        recs = [(i * h * w * 3, h, w) for i in range(n)]
    if len(paths) != len(recs):
        raise ValueError(f"{len(recs)} images, {len(paths)} paths")
    for d in {os.path.dirname(p) for p in paths}:
        if d:
            os.makedirs(d, exist_ok=True)

    def one(i):
        o, h, w = recs[i]
        with open(paths[i], "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (w, h))
            f.write(memoryview(host[o:o + h * w * 3]))

    workers = int(threads) if threads else min(8, len(recs))
    if workers <= 1:
        for i in range(len(recs)):
            one(i)
    else:
        with ThreadPoolExecutor(workers) as pool:
            list(pool.map(one, range(len(recs))))


def cv_resize(x, size):
    """``cv2.resize(img, (w, h))`` (default INTER_LINEAR) of an [n, h, w, c]
    uint8 device batch (c <= 4): the clean image of the 08 PSNR leg
    (08:118-119; OpenCV's fixed-point bilinear, not PIL's, see
    rr_cv_resize_linear_u8).  ``size`` = (w, h) in cv2's order.  A
    ``RaggedBatch`` is resized image by image, each from its own size, in one
    launch (``RaggedBatch.cv_resize``)."""
    if isinstance(x, RaggedBatch):
        return x.cv_resize(size)
    _check_u8(x)
    ow, oh = size
    return ops.cv_resize_linear_u8(x, oh, ow)


def psnr(a, b):
    """per-image PSNR (08:123, data_range 255) of [n, h, w, c] uint8 batches"""
    return ops.psnr_u8(a, b)


def ssim(a, b):
    """per-image SSIM (08:125, data_range 255, channel_axis=2)"""
    return ops.ssim_u8(a, b)


def restoration_quality(clean, restored):
    """The metric leg of the 08 loop for a batch (08:118-125) -> ``(psnr,
    ssim)``, fp64 [n] each, of every restored image against its clean original.

    ``restored``: [n, oh, ow, c] uint8 device tensor (``rr_to_uint8_hwc``'s
    layout).  ``clean``: a ``RaggedBatch`` of the n originals at their own
    sizes -- each is put through ``cv2.resize(clean, (ow, oh))`` (08:118-119)
    and compared in one fused call of two launches, the resized clean images
    never written to memory (``ops.eval_ragged_u8``) -- or a dense uint8 tensor
    of ``restored``'s shape, compared as it is by ``psnr`` and ``ssim``.

    The two arguments must share one channel order (08 compares BGR with BGR;
    RGB with RGB gives the same PSNR, and an SSIM whose channel mean differs in
    the last bit at most).  Anything else raises ``TypeError``; a batch or
    channel count that differs between the two raises ``ValueError``."""
    if (not isinstance(restored, torch.Tensor) or restored.dtype != torch.uint8 or restored.dim() != 4
            or not restored.is_cuda):
        raise TypeError("restoration_quality: restored must be an [n, oh, ow, c] uint8 device tensor")
    if isinstance(clean, RaggedBatch):
        if not clean.data.is_cuda:
            raise TypeError("restoration_quality: the clean RaggedBatch must lie on the device")
        if len(clean) != restored.shape[0] or clean.channels != restored.shape[3]:
            raise ValueError(f"restoration_quality: {len(clean)} clean images of {clean.channels} channels "
                             f"against restored {tuple(restored.shape)}")
        return ops.eval_ragged_u8(clean.data, clean.table, clean.max_hw, clean.channels, restored)
    if (not isinstance(clean, torch.Tensor) or clean.dtype != torch.uint8 or clean.dim() != 4
            or not clean.is_cuda):
        raise TypeError("restoration_quality: clean must be a RaggedBatch or an [n, oh, ow, c] uint8 "
                        "device tensor")
    if clean.shape[0] != restored.shape[0] or clean.shape[3] != restored.shape[3]:
        raise ValueError(f"restoration_quality: clean {tuple(clean.shape)} against restored "
                         f"{tuple(restored.shape)}")
    if clean.shape != restored.shape:
        raise TypeError(f"restoration_quality: a dense clean batch must have restored's shape "
                        f"{tuple(restored.shape)}, not {tuple(clean.shape)} (pass a RaggedBatch to resize)")
    return psnr(clean, restored), ssim(clean, restored)


# ---------------------------------------------------------------------------
# PNG output (17:89-99)

def _host_u8(images):
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] not in (1, 3):
        raise ValueError("expected an [n, h, w, 1|3] uint8 tensor (rr_to_uint8_hwc layout)")
    return images.contiguous().cpu() if images.is_cuda else images.contiguous()


def encode_png(image, level=1):
    """One [h, w, c] uint8 RGB (or greyscale) image -> PNG bytes."""
    if image.dim() == 3:
        image = image.unsqueeze(0)
    host = _host_u8(image)
    _, h, w, c = host.shape
    need = lib().rr_png_encode(h, w, c, host.data_ptr(), int(level), None, 0)
    if need < 0:
        lib().check(int(need), "rr_png_encode")
    buf = (C.c_uint8 * need)()
    got = lib().rr_png_encode(h, w, c, host.data_ptr(), int(level), C.addressof(buf), need)
    if got != need:
        lib().check(int(got) if got < 0 else -1, "rr_png_encode")
    return bytes(buf)


def write_png(images, paths, level=1, threads=0):
    """Batched PNG writer for restored images (17:89-99).  ``images``: the
    [n, h, w, 3] uint8 RGB batch of ops.to_uint8_hwc (device or host).  The
    reference swaps to BGR and calls cv2.imwrite, which writes the RGB pixels
    back out; the files here hold the same RGB pixels.  Parent directories are
    created (17:96)."""
    host = _host_u8(images)
    n, h, w, c = host.shape
    paths = [os.fspath(p) for p in paths]
    if len(paths) != n:
        raise ValueError(f"{n} images, {len(paths)} paths")
    for p in paths:
        d = os.path.dirname(p)
        if d:
            os.makedirs(d, exist_ok=True)
    arr = (C.c_char_p * max(n, 1))(*[p.encode() for p in paths])
    lib().check(lib().rr_png_write_batch(n, h, w, c, host.data_ptr(), C.cast(arr, C.c_void_p),
                                         int(level), int(threads)), "rr_png_write_batch")
