"""The guide preparation the two image-space restatements share
(tests/post_ref.py, as the kernels share csrc/rt_post.h), pinned on a frame
small enough to work out by hand."""
import numpy as np

import denoise_ref
import post_ref
import temporal_ref

F = np.float32
SPP = 4


def test_guide_preparation_on_a_hand_written_frame():
    """2x2 at 4 spp: a sky pixel (whose sums are not looked at), a pixel whose
    normals cancel (hits 2 < spp), a fully covered pixel (hits = spp) and a
    partially covered one (hits 3): n, P and sky are these arrays, bit for bit,
    from post_ref.guides and from both restatements' prepare."""
    hits = np.array([[0, 2], [4, 3]], np.uint32)
    normal = np.array([[[1, 2, 3], [0, 0, 0]], [[0, 0, 8], [9, 0, 12]]], F)
    position = np.array([[[5, 6, 7], [2, 4, -6]], [[4, 8, 12], [1.5, -3, 6]]], F)
    want_n = np.array([[[0, 0, 0], [0, 0, 0]], [[0, 0, 1], [0.6, 0, 0.8]]], F)
    want_P = np.array([[[0, 0, 0], [1, 2, -3]], [[1, 2, 3], [0.5, -1, 2]]], F)
    want_sky = np.array([[True, False], [False, False]])
    colour = np.full((2, 2, 3), 2.0, F)
    for n, P, sky in (post_ref.guides(normal, position, hits),
                      denoise_ref.prepare(colour, hits, position, normal, colour, SPP)[1:4],
                      temporal_ref.prepare(colour, hits, position, normal, SPP)[1:4]):
        assert n.dtype == F and P.dtype == F and sky.dtype == bool
        assert n.tobytes() == want_n.tobytes(), n
        assert P.tobytes() == want_P.tobytes(), P
        assert np.array_equal(sky, want_sky)
