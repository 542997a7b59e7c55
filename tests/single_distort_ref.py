"""numpy restatement of the single distortions of the offline generators, as
the reference spells them -- TEST INFRASTRUCTURE ONLY:

* ``noise``      02_gen_noise.py:18-26 (``low=-1.0``; the branch-free form, see
  ``noise_literal``) and 13_pipeline_stress_test.py:33-38 (``low=0.0``)
* ``blur``       03_gen_blur.py:17-30 (``stretch=True``) and 13:40-48
* ``normalize``  cv2.normalize(src, dst, 0, 255, NORM_MINMAX) on uint8
* ``fog``        04_gen_fog.py:17-30 and 13:50-56, ``t`` an argument
* ``chain13``    13's blur -> fog -> noise, each step fp64 -> uint8

cv2 is absent here, so three things stay parity-unpinned: convertTo's
multiply-add (which OpenCV's SIMD build may fuse), the filter at 144 taps
(which OpenCV may run through its DFT path) and numpy's out-of-range cast to
uint8 (it wraps on the numpy this was written against; the wrap is written
out below so that the restatement does not depend on it)."""
import warnings

import numpy as np

from oracle.imgproc_cpu import filter2d_u8, motion_blur_kernel

A_FOG = 0.9


def wrap_u8(v):
    """np.uint8(v) of an fp64 array in [-255, 255]: toward zero, then modulo 256"""
    return (np.trunc(v).astype(np.int64) & 255).astype(np.uint8)


def noise(img, nz, low=-1.0):
    """02:18-26 with the field ``nz`` as an argument.  02:21-25 picks the lower
    clip from ``out.min() < 0``; when no element is negative the clip is inert
    either way, so ``low=-1.0`` is the reference for every image."""
    out = np.array(img / 255, dtype=float) + nz
    return wrap_u8(np.clip(out, low, 1.0) * 255)


def noise_literal(img, nz):
    """02:18-26 word for word, np.uint8 included"""
    image = np.array(img / 255, dtype=float)
    out = image + nz
    if out.min() < 0:
        low_clip = -1.
    else:
        low_clip = 0.
    out = np.clip(out, low_clip, 1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with np.errstate(all="ignore"):
            out = np.uint8(out * 255)
    return out


def normalize(img):
    """cv2.normalize(img, img, 0, 255, cv2.NORM_MINMAX) on a uint8 image: the
    minimum and maximum over all channels together, scale and shift in fp64,
    convertTo in fp32 with saturate_cast<uchar> (round half to even)"""
    smin, smax = float(img.min()), float(img.max())
    scale = 255.0 * (1.0 / (smax - smin) if smax - smin > np.finfo(np.float64).eps else 0.0)
    shift = 0.0 - smin * scale
    v = (img.astype(np.float32) * np.float32(scale)).astype(np.float32) + np.float32(shift)
    return np.clip(np.rint(v.astype(np.float32)), 0, 255).astype(np.uint8)


def blur(img, degree=10, angle=45, stretch=True):
    """03:17-30; ``stretch=False``: 13:40-48"""
    out = filter2d_u8(img, motion_blur_kernel(degree, angle))
    return normalize(out) if stretch else out


def fog(img, t, A=A_FOG):
    """04:17-30 with its draw as an argument (13:50-56: t = 0.9)"""
    image = np.array(img) / 255.0
    fog_img = image * t + A * (1 - t)
    return np.clip(fog_img * 255, 0, 255).astype(np.uint8)


def chain13(img, nz):
    """13:33-56 as 13 applies it: blur(5, 45) -> fog(0.1) -> noise(var 0.01, clip at 0)"""
    x = blur(img, 5, 45, stretch=False)
    x = fog(x, 1.0 - 0.1)
    return noise(x, nz, low=0.0)
