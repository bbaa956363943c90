"""ti_wpack_kq_host (bits 4 | BITS_G32 | BITS_KQ): tiles and 16-byte scale entries byte for byte against a NumPy
restatement of the layout (include/ti_hip.h), 4.5 bits per weight, and no K that is not whole super-blocks."""
import numpy as np
import pytest


def kq_blocks(rng, K, N):   # q [K][N] 0..15, sc and m [K/32][N] 0..63, d and dmin fp16 [K/256][N]
    d, dmin = ((rng.uniform(0.5, 2.0, (K // 256, N)) * s).astype(np.float16) for s in (1e-3, 8e-3))
    return (rng.randint(0, 16, (K, N)).astype(np.uint8), rng.randint(0, 64, (K // 32, N)).astype(np.uint8),
            rng.randint(0, 64, (K // 32, N)).astype(np.uint8), d, dmin)


def unpack(tiles, scales, K, N):
    """The layout read back as (q, sc, m, d, dmin): every bit lands in exactly one field, so equal fields are equal bytes."""
    t = np.ascontiguousarray(tiles).view(np.uint32).reshape(N // 16, K // 128, 4, 16, 4)   # [nt][g][kq][r][s4]
    nib = np.stack([(t >> (16 + 4 * (e >> 1) if e & 1 else 4 * (e >> 1))) & 15 for e in range(8)], axis=-1)
    q = nib.transpose(1, 4, 2, 5, 0, 3).reshape(K, N).astype(np.uint8)   # k = 128 g + 32 s4 + 8 kq + e, n = 16 nt + r
    ent = np.ascontiguousarray(scales).view(np.uint32).reshape(N // 16, K // 256, 16, 4).astype(np.uint64)   # [nt][sb][r][word]
    bits96 = [int(a) | int(b) << 32 | int(c) << 64 for a, b, c in ent[..., 1:].reshape(-1, 3)]
    fld = np.array([[v >> 6 * f & 63 for f in range(16)] for v in bits96], np.uint8).reshape(N // 16, K // 256, 16, 8, 2)
    sc, m = (fld[..., i].transpose(1, 3, 0, 2).reshape(K // 32, N) for i in range(2))   # field 2 j: sc_j, 2 j + 1: m_j
    d, dmin = ((ent[..., 0] >> s & 0xffff).astype(np.uint16).view(np.float16).transpose(1, 0, 2).reshape(K // 256, N) for s in (0, 16))
    return q, sc, m, d, dmin


@pytest.mark.parametrize("K,N", [(256, 16), (512, 48)])
@pytest.mark.parametrize("row_map", [0, 1])
def test_wpack_kq_layout(ti_host, K, N, row_map):
    T, rng = ti_host, np.random.RandomState(K + N + row_map)
    n_total, offs = ((2 * N, (0, 8)) if row_map else (N + 16, (16,)))
    want = [np.zeros((r, n_total), t) for r, t in ((K, np.uint8), (K // 32, np.uint8), (K // 32, np.uint8), (K // 256, np.float16), (K // 256, np.float16))]
    tiles = scales = None
    for off in offs:
        blk, c = kq_blocks(rng, K, N), np.arange(N)
        for w, a in zip(want, blk):
            w[:, 16 * (c >> 3) + (c & 7) + off if row_map else off + c] = a
        tiles, scales = T.wpack_kq(*blk, n_total, row_map, off, tiles, scales)
    for w, g in zip(want, unpack(tiles, scales, K, n_total)):
        assert np.array_equal(w.view(np.uint16) if w.dtype == np.float16 else w, g.view(np.uint16) if g.dtype == np.float16 else g)
    sizes = [f(4 | T.BITS_G32 | T.BITS_KQ, K, n_total) for f in (T.lib().ti_wpack_tile_bytes, T.lib().ti_wpack_scale_bytes)]
    assert [len(tiles), len(scales)] == sizes and sum(sizes) == K * n_total * 9 // 16


def test_wpack_kq_refuses_half_a_super_block(ti_host):
    q, sc, m, d, dmin = kq_blocks(np.random.RandomState(0), 512, 16)
    with pytest.raises(ti_host.TiError):   # 384 = 1.5 super-blocks
        ti_host.wpack_kq(q[:384], sc[:12], m[:12], d, dmin)
