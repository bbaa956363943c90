"""MXFP4 packing on the host (bits 4 | BITS_G32 | BITS_MX): ti_wpack_mx_host's tiles and e8m0 scale bytes byte for
byte against a NumPy restatement of the layout (include/ti_hip.h), ti_wpack_host's quantization against a NumPy
statement of the OCP rule, and the argument errors of a block scale outside [1, 254]."""
import numpy as np
import pytest

GRID = np.array([0, .5, 1, 1.5, 2, 3, 4, 6])


def layout(parts, K, n_total, row_map):
    """(tiles u32 [N/16][K/128][64 lanes][4], scales u8 [N/16][K/128][4][16]) of [(codes, e, row_offset), ..]."""
    KT = K // 128
    tiles, scales = np.zeros((n_total // 16, KT, 64, 4), np.uint32), np.zeros((n_total // 16, KT, 4, 16), np.uint8)
    for codes, e, off in parts:
        c = np.arange(codes.shape[1])
        n = 16 * (c >> 3) + (c & 7) + off if row_map else off + c
        zero = ~(codes.reshape(K // 32, 32, -1) & 7).any(axis=1)
        for g in range(KT):
            for s4 in range(4):
                scales[n >> 4, g, s4, n & 15] = np.where(zero[4 * g + s4], 127, e[4 * g + s4])
                for kq in range(4):
                    for el in range(8):   # lane 16 kq + row, word s4: k = 32 s4 + 8 kq + el
                        sh = 16 + 4 * (el >> 1) if el & 1 else 4 * (el >> 1)
                        tiles[n >> 4, g, 16 * kq + (n & 15), s4] |= codes[128 * g + 32 * s4 + 8 * kq + el].astype(np.uint32) << sh
    return tiles.reshape(-1).view(np.uint8), scales.reshape(-1)


@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("row_map", [0, 1])
def test_wpack_mx_layout(ti_host, K, N, row_map):
    T, rng = ti_host, np.random.RandomState(K + N + row_map)
    n_total, offs = ((2 * N, (0, 8)) if row_map else (N + 16, (16,)))
    parts = [(rng.randint(0, 16, (K, N)).astype(np.uint8), rng.randint(1, 255, (K // 32, N)).astype(np.uint8), o) for o in offs]
    parts[0][0][32:64, 3] &= 8   # a block of +-0 codes: 127 is stored whatever e says
    tiles = scales = None
    for codes, e, off in parts:
        tiles, scales = T.wpack_mx(codes, e, n_total, row_map, off, tiles, scales)
    want_t, want_s = layout(parts, K, n_total, row_map)
    assert np.array_equal(tiles, want_t) and np.array_equal(scales, want_s)
    assert len(scales) == n_total * K // 32 == T.lib().ti_wpack_scale_bytes(4 | T.BITS_G32 | T.BITS_MX, K, n_total)


def mx_quantize(w):
    """The OCP rule: e = floor(log2(absmax)) - 2 + 127 in [1, 254] (127 for a zero block), code = sign | nearest-even
    e2m1 magnitude of |w| / 2^(e - 127), saturating at 6."""
    K, N = w.shape
    b = w.astype(np.float64).reshape(K // 32, 32, N)
    amax = np.abs(b).max(axis=1)
    e = np.where(amax > 0, np.clip(np.frexp(amax)[1] - 1 - 2 + 127, 1, 254), 127)
    v = np.abs(b) / 2.0 ** (e - 127)[:, None, :]
    mids = (GRID[:-1] + GRID[1:]) / 2
    code = sum(((v > m) | ((v == m) & bool(i & 1))).astype(np.uint8) for i, m in enumerate(mids))
    return (code | np.where(b < 0, 8, 0).astype(np.uint8)).reshape(K, N), e.astype(np.uint8)


def test_wpack_host_mx_rule(ti_host):
    T, K, N = ti_host, 256, 16
    rng = np.random.RandomState(1)
    w = (rng.standard_normal((K, N)) * np.exp2(rng.randint(-20, 12, (K // 32, N))).repeat(32, axis=0)).astype(np.float32)
    w[0:32, 0] = 0                                                                  # an all-zero block
    w[32:64, 1] = np.clip(w[32:64, 1], -0.2, 0.2); w[40, 1] = 0.25                  # absmax exactly a power of two
    ties = np.array([.25, .75, 1.25, 1.75, 2.5, 3.5, 5.0], np.float32)              # every tie, both signs, at scale 1
    w[64:96, 2] = 0; w[64:71, 2] = ties; w[71:78, 2] = -ties; w[78, 2] = 6.0
    w[96:128, 3] = np.linspace(-7.9, 7.9, 32)                                       # absmax 7.9: e = 127, 7.9 -> 6
    codes, e = mx_quantize(w)
    assert e[0, 0] == 127 and e[1, 1] == 123 and e[2, 2] == 127 and e[3, 3] == 127
    assert codes[64:71, 2].tolist() == [0, 2, 2, 4, 4, 6, 6] and codes[96, 3] == 15 and codes[127, 3] == 7
    tiles, scales = T.wpack_host(w, 4 | T.BITS_G32 | T.BITS_MX)
    want_t, want_s = T.wpack_mx(codes, e)
    assert np.array_equal(tiles, want_t) and np.array_equal(scales.view(np.uint8)[:len(want_s)], want_s)


@pytest.mark.parametrize("e", [0, 255])
def test_wpack_mx_refuses_scales_outside_the_format(ti_host, e):
    T = ti_host
    codes, scales = np.zeros((128, 16), np.uint8), np.full((4, 16), 120, np.uint8)
    scales[2, 5] = e
    assert T.wpack_mx(codes, scales)[1].reshape(4, 16)[2, 5] == 127   # a zero block may carry any e
    codes[70, 5] = 9
    with pytest.raises(T.TiError):
        T.wpack_mx(codes, scales)
