"""The dead-plane table of the Winograd kernel's transposed-convolution forms (csrc/conv_wino.hip: wino_dead_forms, pack_deconv_wino),
on the CPU.

ConvTranspose2d(4, 2, 1) as a 3x3 layer has, per output parity (py, px), taps in rows {py, py + 1} and columns {px, px + 1} only, so
U = G g G^T has plane row 3 (py = 0) or 0 (py = 1) and plane column 3 (px = 0) or 0 (px = 1) exactly zero.  The library finds that in the
PACKED weights, block by block, and the kernel skips the row or column a 32-channel N block shares.  Checked here: the forms for the
channel counts the models use, that only exact zeros count (dense layers, half-padded blocks, a NaN), and that the order of the parity
groups the pack chooses is the one the kernel's epilogue decodes.
"""
import ctypes as C

import numpy as np
import pytest

NONE, ROW0, ROW3, COL0, COL3 = 0, 1, 2, 3, 4


def _rand(shape, seed):
    return (np.random.default_rng(seed).random(shape, dtype=np.float32) * 2 - 1).astype(np.float32)


def _forms(lib, w3, cin_p=None):
    """forms of a 3x3 layer w3 [Cout][Cin][3][3] as the library's scan of its own pack reports them"""
    w3 = np.ascontiguousarray(w3, np.float32)
    cout, cin = w3.shape[:2]
    out = (C.c_int * 32)()
    n = lib.vfi_test_wino_dead_forms(w3.ctypes.data, cout, cin, cin_p or cin, out, 32)
    assert n == (cout + 31) // 32, n
    return tuple(out[:n])


def _plan(lib, w, lo):
    """(forms, gray, order) of a transposed layer w [Cin][LO][4][4]"""
    w = np.ascontiguousarray(w, np.float32)
    forms, gray, order = (C.c_int * 32)(), C.c_int(-1), (C.c_int * (4 * lo))()
    n = lib.vfi_test_deconv_wino_plan(w.ctypes.data, w.shape[0], lo, forms, 32, C.byref(gray), order)
    assert n == (4 * lo + 31) // 32, n
    return tuple(forms[:n]), gray.value, list(order)


def _w3(lib, w, lo):
    """the library's own 3x3 embedding (pack_deconv_as_conv3x3): [4 * LO][Cin][3][3], channel g * LO + co, g = 2 py + px"""
    w = np.ascontiguousarray(w, np.float32)
    cin = w.shape[0]
    w3, b3 = np.zeros((4 * lo, cin, 3, 3), np.float32), np.zeros(4 * lo, np.float32)
    assert lib.vfi_test_pack_deconv3x3(w.ctypes.data, None, cin, lo, w3.ctypes.data, b3.ctypes.data, w3.size) == w3.size
    return w3


def test_zero_rows_and_columns_of_u_per_parity(hip_lib):
    """the premise, in float64 numpy on the library's embedding: U = G g G^T of parity (py, px) has row 3 - 3 py and column 3 - 3 px zero
    and nothing else (dense random taps), so 9 of 16 planes are live"""
    G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
    lo = 3
    w3 = _w3(hip_lib, _rand((8, lo, 4, 4), 1), lo).astype(np.float64)
    for g in range(4):
        py, px = g >> 1, g & 1
        U = np.einsum("ri,ocij,sj->ocrs", G, w3[g * lo:(g + 1) * lo], G)
        zero = (U == 0).all(axis=(0, 1))
        want = np.zeros((4, 4), bool)
        want[3 - 3 * py, :] = True
        want[:, 3 - 3 * px] = True
        assert (zero == want).all(), (g, zero)
        assert int((~zero).sum()) == 9


def test_lo24_takes_the_gray_order(hip_lib):
    """RIFE's lastconv: 4 x 24 channels = 3 blocks.  p00 p01 p10 p11 would leave block 1 (p01 + p10) with no common row or column; in
    the order p00 p01 p11 p10 it is pure px = 1: (row 3, column 0, row 0) = 12 of 48 planes"""
    forms, gray, order = _plan(hip_lib, _rand((16, 24, 4, 4), 2), 24)
    assert gray == 1 and forms == (ROW3, COL0, ROW0)
    assert order[:48] == list(range(48)) and order[48:72] == list(range(72, 96)) and order[72:] == list(range(48, 72))
    # ... and what the plain order would give, from the scan of the plain embedding: only two of the four dead planes of block 1's
    # groups coincide, which is no form
    assert _forms(hip_lib, _w3(hip_lib, _rand((16, 24, 4, 4), 2), 24)) == (ROW3, NONE, ROW0)


@pytest.mark.parametrize("lo,want", [(16, (ROW3, ROW0)), (32, (ROW3, ROW3, ROW0, ROW0))])
def test_pure_py_blocks_keep_the_plain_order(hip_lib, lo, want):
    """LO = 16 / 32 (M2M, IFRNet, GMFSS): every block is one py group — row forms, a row before a column, no reordering (the Gray
    order is taken only where it skips MORE planes)"""
    forms, gray, order = _plan(hip_lib, _rand((8, lo, 4, 4), 3), lo)
    assert forms == want and gray == 0 and order == list(range(4 * lo))


def test_lo52_seven_blocks(hip_lib):
    """RIFE 4.26's lastconv: 208 channels in 7 blocks.  Block 3 spans p01 | p10 in the plain order (no form) and p01 | p11 in the Gray
    order (column 0); block 6 is 16 channels of one group + 16 of padding, whose zeros do not hide the group's live planes"""
    forms, gray, _ = _plan(hip_lib, _rand((8, 52, 4, 4), 3), 52)
    assert gray == 1 and forms == (ROW3, ROW3, ROW3, COL0, ROW0, ROW0, ROW0)


def test_dense_and_half_padded_layers_have_no_form(hip_lib):
    assert _forms(hip_lib, _rand((64, 8, 3, 3), 4)) == (NONE, NONE)
    # Cout = 40 padded to 64: block 1 is 8 live channels + 24 of padding — the zeros of the padding alone make no plane dead
    assert _forms(hip_lib, _rand((40, 8, 3, 3), 5)) == (NONE, NONE)
    # padded INPUT channels (Cin 5 of 8) neither
    assert _forms(hip_lib, _rand((32, 5, 3, 3), 6), cin_p=8) == (NONE,)


def test_a_nan_keeps_its_block_alive(hip_lib):
    lo = 24
    w3 = _w3(hip_lib, _rand((8, lo, 4, 4), 7), lo)
    w3 = w3[[c if c < 48 else (c + 24 if c < 72 else c - 24) for c in range(96)]]      # the Gray order, restated
    assert _forms(hip_lib, w3) == (ROW3, COL0, ROW0)
    for co, (ky, kx) in ((5, (2, 1)), (40, (1, 0)), (90, (0, 2))):      # one zero tap of a would-be dead row / column per block
        bad = w3.copy()
        assert bad[co, 3, ky, kx] == 0
        bad[co, 3, ky, kx] = np.nan
        want = [ROW3, COL0, ROW0]
        want[co // 32] = NONE
        assert _forms(hip_lib, bad) == tuple(want), co
    tiny = w3.copy()
    tiny[5, 3, 2, 1] = np.float32(1e-30)      # ... and so does any non-zero weight, however small
    assert _forms(hip_lib, tiny) == (NONE, COL0, ROW0)      # row 3 of block 0 lives, and p00 | p01 share no column


@pytest.mark.parametrize("lo", [1, 4, 13, 16, 24, 32, 52, 256])
def test_order_then_epilogue_decode_is_the_identity(hip_lib, lo):
    """N position co holds row order[co] of the embedding (channel g * LO + cg of parity g = 2 py + px); the kernel's SHUF epilogue
    decodes g from the POSITION — co / LO by float multiplication with one fix-up step, then g ^= g >> 1 under the Gray order —
    and must arrive at that parity and channel for every co"""
    _, gray, order = _plan(hip_lib, _rand((8, lo, 4, 4), 8), lo)
    assert sorted(order) == list(range(4 * lo))
    inv = np.float32(1.0) / np.float32(lo)
    for co in range(4 * lo):
        g = int(np.float32(co) * inv)
        cg = co - g * lo
        if cg < 0:
            g, cg = g - 1, cg + lo
        if cg >= lo:
            g, cg = g + 1, cg - lo
        g ^= (g >> 1) & gray
        assert (g, cg) == divmod(order[co], lo), co
    if lo == 24:
        assert gray == 1


def test_the_hooks_are_test_taps_only(hip_lib):
    """include/vfi_hip_test_wino.h: bound in the test build, absent from the product library (dlopen only, no call)"""
    from cfi_amd import _lib

    product = C.CDLL(_lib.LIB_PATH)
    for name in _lib.WINO_TEST_PROTOTYPES:
        assert getattr(hip_lib, name) is not None and not hasattr(product, name), name
