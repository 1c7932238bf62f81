"""functional._conv_route / _convt_route: which kernels a convolution of the autograd front end runs on, as a table of geometry
against route.  The expected column was read off the four convolution Functions (_Conv5, _ConvT5, _ConvT4, _ConvK) that the two
route functions replace, condition by condition -- one row per route and sub-choice and the near-miss next to each condition; it
is not computed by the functions under test.  No device is needed: the only library calls are two host-side workspace queries
(rows marked LIB; they are skipped when the library is not built)."""
import os

import pytest

from vae_play_amd import _lib
from vae_play_amd import functional as F

NONE, RELU, TANH, SIGMOID = 0, 1, 3, 4
LIB = True

# (precision, _SMALL3, _SMALL3_ALL, Cout, Cin, ks, stride, act, bias, H, W) -> (forward, input gradient, weight gradient); B = 2
CONV5 = [
    # im2col: bf16x3, stride 2, 1 | 3 channels in, Cout % 8 == 0, no activation, no bias, even image
    (("bf16x3", True, True, 8, 1, 5, 2, NONE, False, 8, 8), ("im2col", "scatter_padded", "im2col")),
    (("bf16x3", True, True, 64, 3, 5, 2, NONE, False, 8, 8), ("im2col", "scatter_padded", "im2col")),
    (("bf16x3", True, True, 8, 3, 5, 2, NONE, False, 7, 8), ("f32", "scatter_padded", "f32")),           # odd H
    (("bf16x3", True, True, 8, 3, 5, 2, NONE, False, 8, 7), ("f32", "scatter_padded", "f32")),           # odd W
    (("bf16x3", True, True, 8, 1, 5, 2, NONE, True, 8, 8), ("f32", "scatter_padded", "f32")),            # bias
    (("bf16x3", True, True, 8, 1, 5, 2, RELU, False, 8, 8), ("f32", "scatter_padded", "f32")),           # activation
    (("bf16x3", True, True, 12, 3, 5, 2, NONE, False, 8, 8), ("f32", "f32", "f32")),                     # Cout % 8 != 0
    (("bf16x3", True, True, 8, 2, 5, 2, NONE, True, 8, 8), ("f32", "scatter_padded", "f32")),            # 2 channels in
    (("bf16x3", True, True, 8, 3, 5, 1, NONE, False, 8, 8), ("f32", "scatter_padded", "f32")),           # stride 1
    (("f32", True, True, 8, 1, 5, 2, NONE, False, 8, 8), ("f32", "f32", "f32")),
    # smallin: first_conv_s1_edge (bf16x3, stride 1, 1 | 3 in, 32 | 64 out) and no activation | ReLU
    (("bf16x3", True, True, 32, 1, 5, 1, RELU, True, 8, 8), ("smallin", "smallout_flipped", "f32")),
    (("bf16x3", True, True, 64, 3, 5, 1, NONE, False, 8, 8), ("smallin", "smallout_flipped", "f32")),
    (("bf16x3", True, True, 32, 1, 5, 1, SIGMOID, True, 8, 8), ("f32", "smallout_flipped", "f32")),      # activation
    (("bf16x3", True, True, 16, 3, 5, 1, NONE, False, 8, 8), ("f32", "scatter_padded", "f32")),          # Cout = 16
    (("bf16x3", True, True, 32, 2, 5, 1, RELU, True, 8, 8), ("f32", "scatter_padded", "f32")),           # 2 channels in
    (("bf16x3", True, True, 32, 1, 5, 2, RELU, True, 8, 8), ("f32", "scatter_padded", "f32")),           # stride 2
    (("f32", True, True, 32, 1, 5, 1, RELU, True, 8, 8), ("f32", "f32", "f32")),
    # x16: bf16x3, both channel counts % 8 == 0, no activation | sigmoid
    (("bf16x3", True, True, 16, 8, 5, 2, NONE, False, 8, 8), ("x16", "x16", "x16")),
    (("bf16x3", True, True, 64, 64, 5, 1, SIGMOID, True, 7, 9), ("x16", "x16", "x16")),
    (("bf16x3", True, True, 16, 8, 5, 2, RELU, False, 8, 8), ("f32", "f32", "f32")),                     # ReLU
    (("bf16x3", True, True, 16, 8, 5, 2, TANH, False, 8, 8), ("f32", "f32", "f32")),
    (("bf16x3", True, True, 16, 12, 5, 2, NONE, False, 8, 8), ("f32", "f32", "f32")),                    # Cin % 8 != 0
    (("bf16x3", True, True, 12, 16, 5, 2, NONE, False, 8, 8), ("f32", "f32", "f32")),                    # Cout % 8 != 0
    (("f32", True, True, 16, 8, 5, 2, NONE, False, 8, 8), ("f32", "f32", "f32")),
    # smallout: bf16x3, stride 1, 64 in, 1 | 3 out, no activation | sigmoid; its weight-gradient kernel where its query says so
    (("bf16x3", True, True, 1, 64, 5, 1, SIGMOID, True, 8, 8), ("smallout", "smallin_dgrad", "f32"), LIB),
    (("bf16x3", True, True, 3, 64, 5, 1, NONE, False, 16, 64), ("smallout", "smallin_dgrad", "smallout_wgrad"), LIB),
    (("bf16x3", True, True, 1, 64, 5, 1, SIGMOID, True, 16, 48), ("smallout", "smallin_dgrad", "f32"), LIB),   # W % 64 != 0
    (("bf16x3", True, True, 2, 64, 5, 1, SIGMOID, True, 16, 64), ("f32", "halo_padded", "f32")),         # Cout = 2
    (("bf16x3", True, True, 1, 32, 5, 1, SIGMOID, True, 16, 64), ("f32", "halo_padded", "f32")),         # Cin = 32
    (("bf16x3", True, True, 1, 64, 5, 1, RELU, True, 16, 64), ("f32", "halo_padded", "f32")),            # ReLU
    (("bf16x3", True, True, 1, 64, 5, 2, SIGMOID, True, 16, 64), ("f32", "f32", "f32")),                 # stride 2
    (("f32", True, True, 1, 64, 5, 1, SIGMOID, True, 16, 64), ("f32", "f32", "f32")),
    # input-gradient sub-choices of the f32 forward route: halo_padded (Cout < 8, Cin % 8 == 0, stride 1), smallout_flipped
    # (1 | 3 in, 32 | 64 out, stride 1), scatter_padded (Cin < 8, Cout % 8 == 0)
    (("bf16x3", True, True, 3, 16, 5, 1, NONE, False, 8, 8), ("f32", "halo_padded", "f32")),
    (("bf16x3", True, True, 3, 12, 5, 1, NONE, False, 8, 8), ("f32", "f32", "f32")),                     # Cin % 8 != 0
    (("bf16x3", True, True, 3, 16, 5, 2, NONE, False, 8, 8), ("f32", "f32", "f32")),                     # stride 2
    (("f32", True, True, 3, 16, 5, 1, NONE, False, 8, 8), ("f32", "f32", "f32")),
    (("bf16x3", True, True, 64, 1, 5, 1, TANH, False, 8, 8), ("f32", "smallout_flipped", "f32")),
    (("f32", True, True, 64, 1, 5, 1, TANH, False, 8, 8), ("f32", "f32", "f32")),
    (("bf16x3", True, True, 16, 3, 5, 2, NONE, True, 8, 8), ("f32", "scatter_padded", "f32")),
    (("bf16x3", True, True, 12, 3, 5, 2, NONE, True, 8, 8), ("f32", "f32", "f32")),                      # Cout % 8 != 0
    (("f32", True, True, 16, 3, 5, 2, NONE, True, 8, 8), ("f32", "f32", "f32")),
]

CONV2D = [
    # small3: _SMALL3, 3x3, stride 1 and the kernel's own query (few channels on both sides); in both precisions
    (("f32", True, True, 4, 8, 3, 1, NONE, True, 8, 8), ("small3", "small3", "small3"), LIB),
    (("bf16x3", True, True, 4, 8, 3, 1, NONE, True, 8, 8), ("small3", "small3", "small3"), LIB),
    (("f32", True, False, 4, 8, 3, 1, NONE, True, 8, 8), ("f32", "f32", "small3"), LIB),                  # _SMALL3_ALL = False
    (("bf16x3", True, False, 4, 8, 3, 1, NONE, True, 8, 8), ("padded", "padded", "small3"), LIB),
    (("bf16x3", True, False, 8, 8, 3, 1, NONE, True, 8, 8), ("x16", "x16", "small3"), LIB),
    (("f32", False, True, 4, 8, 3, 1, NONE, True, 8, 8), ("f32", "f32", "f32")),                          # _SMALL3 = False
    (("bf16x3", False, True, 4, 8, 3, 1, NONE, True, 8, 8), ("padded", "padded", "padded")),
    (("f32", True, True, 4, 8, 3, 2, NONE, True, 8, 8), ("f32", "f32", "f32")),                           # stride 2
    (("f32", True, True, 4, 8, 1, 1, NONE, True, 8, 8), ("f32", "f32", "f32")),                           # 1x1
    (("f32", True, True, 16, 16, 3, 1, NONE, True, 8, 8), ("f32", "f32", "f32"), LIB),                    # too many channels
    # padded: bf16x3 and a channel count that is not a multiple of 8
    (("bf16x3", True, True, 16, 10, 3, 1, NONE, True, 8, 8), ("padded", "padded", "padded"), LIB),
    (("bf16x3", False, True, 16, 10, 3, 1, NONE, True, 8, 8), ("padded", "padded", "padded")),
    (("bf16x3", True, True, 1, 16, 1, 1, NONE, True, 8, 8), ("padded", "padded", "padded")),
    (("f32", True, True, 16, 10, 3, 2, NONE, True, 8, 8), ("f32", "f32", "f32")),
    # x16 | f32
    (("bf16x3", True, True, 16, 16, 3, 1, NONE, True, 8, 8), ("x16", "x16", "x16"), LIB),
    (("bf16x3", True, True, 16, 16, 4, 2, NONE, True, 9, 7), ("x16", "x16", "x16")),
    (("f32", True, True, 16, 16, 5, 2, NONE, False, 7, 7), ("f32", "f32", "f32")),
    # the conv5x5 family's special cases are not conv2d's: the same geometries stay on the dense core
    (("bf16x3", True, True, 1, 64, 5, 1, NONE, True, 16, 64), ("padded", "padded", "padded")),
    (("bf16x3", True, True, 8, 1, 5, 2, NONE, False, 8, 8), ("padded", "padded", "padded")),
    (("bf16x3", True, True, 32, 1, 5, 1, NONE, True, 8, 8), ("padded", "padded", "padded")),
]

ROWS = [("conv5x5", *r) for r in CONV5] + [("conv2d", *r) for r in CONV2D]


@pytest.mark.parametrize("family,geom,want,lib", [(r[0], r[1], r[2], len(r) > 3) for r in ROWS],
                         ids=[f"{r[0]}-{'-'.join(map(str, r[1]))}" for r in ROWS])
def test_conv_route(family, geom, want, lib):
    if lib and not os.path.exists(_lib.LIB_PATH):
        pytest.skip("needs a host-side workspace query of the library, which is not built")
    precision, small3, small3_all, Cout, Cin, ks, stride, act, bias, H, W = geom
    got = F._conv_route(precision, small3, small3_all, family, Cout, Cin, ks, stride, act, bias, 2, H, W)
    assert tuple(got) == want


def test_every_route_name_has_a_row():
    fwd = {r[2][0] for r in ROWS}
    dx = {r[2][1] for r in ROWS}
    dw = {r[2][2] for r in ROWS}
    assert fwd == {"im2col", "smallin", "x16", "smallout", "f32", "small3", "padded"}
    assert dx == {"scatter_padded", "smallout_flipped", "x16", "smallin_dgrad", "halo_padded", "f32", "small3", "padded"}
    assert dw == {"im2col", "x16", "smallout_wgrad", "f32", "small3", "padded"}


@pytest.mark.parametrize("precision,Cin,Cout,want", [("bf16x3", 16, 8, "x16"), ("bf16x3", 8, 16, "x16"), ("bf16x3", 16, 3, "f32"),
                                                     ("bf16x3", 4, 4, "f32"), ("bf16x3", 12, 16, "f32"), ("f32", 16, 8, "f32")])
def test_conv_transpose_route(precision, Cin, Cout, want):
    assert F._convt_route(precision, Cin, Cout) == want


def test_first_conv_s1_edge_is_the_smallin_shape():
    import torch
    prev = F.get_conv_precision()
    try:
        F.set_conv_precision("bf16x3")
        assert F.first_conv_s1_edge(torch.empty(32, 1, 5, 5), 1) and F.first_conv_s1_edge(torch.empty(64, 3, 5, 5), 1)
        assert not F.first_conv_s1_edge(torch.empty(32, 1, 5, 5), 2) and not F.first_conv_s1_edge(torch.empty(16, 1, 5, 5), 1)
        assert not F.first_conv_s1_edge(torch.empty(32, 2, 5, 5), 1)
        F.set_conv_precision("f32")
        assert not F.first_conv_s1_edge(torch.empty(32, 1, 5, 5), 1)
    finally:
        F.set_conv_precision(prev)
