"""What the numpy float32 restatements of the image-space passes
(denoise_ref.py, temporal_ref.py, resolve_ref.py, upscale_ref.py) share, as
the kernels share csrc/rt_post.h: the unfused dot product and the guide
preparation from the rt_aov sums.  What the passes that reproject share
(csrc/rt_reproject.h) is temporal_ref.py's project, gather, blend and
pack_history and resolve_ref.py's centre_rays."""
import numpy as np

F = np.float32


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def guides(normal, position, hits):
    """normal, position (H, W, 3) float32 sums, hits (H, W) uint32 -> (n, P,
    sky): the unit mean normal (0 where the mean is 0), the mean position and
    the sky mask (no hits: n and P are 0)."""
    sky = hits == 0
    hf = hits.astype(F)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        n = normal / hf
        nn = _dot(n, n)
        unit = ~sky & (nn > 0)
        n = np.where(unit[..., None], n / np.sqrt(nn)[..., None], F(0)).astype(F)
        P = np.where(sky[..., None], F(0), position / hf).astype(F)
    return n, P, sky
