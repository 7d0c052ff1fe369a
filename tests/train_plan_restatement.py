"""Test-side restatement of the host-side plans of the training kernels, in plain Python: how csrc/conv_train.hip cuts a weight
gradient into shares (wgrad_plan) and a bias gradient into pixel blocks, how csrc/train_head.hip cuts a loss into partials
(head_plan), and the rows of a tile of csrc/ann_train.hip (ann_tile_rows).  A plain helper module.

What it is for.  Each of those kernels has code that runs only when a workgroup takes MORE THAN ONE share: the second and later
units of a share, the second pass of a strided loop, a short last share.  Whether a test shape reaches that code is decided by
these plans, so the GPU tests declare, as data, the regime each of their cases is there for (CONV_REGIMES, HEAD_REGIMES) and
assert it against the restated plan before they launch; tests/test_conv_train_cpu.py and tests/test_head_train_cpu.py pin the
restated plans to the library on a machine without a GPU, through the workspace sizes qgx_conv2d_workspace and
qgx_head_workspace return.  A change of a plan then fails loudly instead of quietly moving a case out of its regime.
"""

GRIDS = (16, 32, 48, 64, 96, 128)


def up(v, m):
    return (v + m - 1) // m * m


def cdiv(a, b):
    return (a + b - 1) // b


# ---- conv_train.hip ----------------------------------------------------------------------------------------------------------
PATCH_STRIDE = 36         # floats per staged pixel
LDS_TWO_PER_CU, LDS_ONE_PER_CU = 80 * 1024, 160 * 1024


def wgrad_lds(R, k, N):
    """bytes of the two LDS patches of a unit of R image rows: R + k - 1 rows of x (with the halo) and R rows of dy"""
    return ((R + k - 1) + R) * N * PATCH_STRIDE * 4


def wgrad_plan(B, N, cin, cout, k):
    """the partition of the weight and bias gradients of one call, and what of it decides which code a workgroup runs"""
    fits = [R for cap in (LDS_TWO_PER_CU, LDS_ONE_PER_CU) for R in (4, 2, 1) if wgrad_lds(R, k, N) <= cap]
    R = fits[0]                                    # the most rows under the small cap, else the most under the large one
    tiles_per_img = N // R
    U = B * tiles_per_img                          # units
    cot_n, cit_n = cdiv(cout, 32), cdiv(cin, 32)
    pairs = cot_n * cit_n
    want = min(cdiv(512, pairs), U)                # shares wanted: about 512 workgroups
    ups = cdiv(U, want)                            # units per share
    S = cdiv(U, ups)
    last_units = U - (S - 1) * ups
    shares = [(s * ups, min(s * ups + ups, U)) for s in range(S)]
    crosses_image = any(u0 // tiles_per_img != (u1 - 1) // tiles_per_img for u0, u1 in shares)
    # db: at most 256 blocks of at least 64 pixels; thread (g, c) of a block adds the pixels p0 + g, p0 + g + G, ...
    npix = B * N * N
    ppb = cdiv(npix, min(npix // 64, 256))
    nb = cdiv(npix, ppb)
    cout8 = up(cout, 8)
    G = 256 // cout8
    return dict(R=R, U=U, ups=ups, S=S, last_units=last_units, tiles_per_img=tiles_per_img, crosses_image=crosses_image,
                cot_n=cot_n, cit_n=cit_n, pairs=pairs, T=k * k, lds=wgrad_lds(R, k, N), under_80k=wgrad_lds(R, k, N) <= LDS_TWO_PER_CU,
                nb=nb, ppb=ppb, last_pixels=npix - (nb - 1) * ppb, G=G, dbias_passes=cdiv(ppb, G), dbias_even=ppb % G == 0)


def packed_floats(ck, cn, T):
    """the weights as the forward engine reads them: T taps x groups of 8 K-channels, one zero group, 32-padded outputs"""
    return (T * (up(ck, 8) // 8) + 1) * up(cn, 32) * 8


def conv_workspace_bytes(B, N, cin, cout, k):
    """the workspace's layout, in floats, every part rounded up to 64: packed weights (of the forward or of the data gradient,
    whichever is larger) | 256 of padded bias | the shares' slices [S][pairs][T][32][32] | db's block sums [nb][cout8]"""
    p = wgrad_plan(B, N, cin, cout, k)
    T = k * k
    floats = up(max(packed_floats(cin, cout, T), packed_floats(cout, cin, T)), 64) + 256
    floats += up(p['S'] * p['pairs'] * T * 1024, 64)
    floats += up(p['nb'] * up(cout, 8), 64)
    return 4 * floats


# the GPU cases that are there for a regime, and the regime as data: every key is asserted against wgrad_plan
CONV_REGIMES = {
    # (cin, cout, k, B, N)
    (1, 256, 3, 34, 16): dict(R=4, ups=3, S=46, last_units=1, pairs=8),
    (40, 70, 5, 23, 16): dict(R=4, cot_n=3, cit_n=2, ups=2, S=46, last_units=2),
    (33, 7, 3, 130, 16): dict(R=4, ups=3, S=174, last_units=1, ppb=130, G=32, dbias_even=False),
    (8, 72, 3, 2, 96): dict(R=1, cot_n=3, ups=2, G=3, ppb=72),
    (8, 8, 3, 9, 96): dict(R=1, ups=2, S=432, ppb=324),
    (8, 8, 3, 9, 128): dict(R=1, lds=73728, ups=3, tiles_per_img=128, crosses_image=True, ppb=576),
    (8, 8, 5, 11, 96): dict(R=2, lds=110592, under_80k=False, ups=2),
    (8, 8, 5, 9, 128): dict(R=2, lds=147456, under_80k=False, ups=2),
    (8, 8, 5, 5, 64): dict(R=2, under_80k=True, ppb=80),
}


def regime_table(cases):
    """one line per case with the plan values that decide a workgroup's path: the table the GPU test prints"""
    lines = ['%-22s %2s %5s %4s %4s %5s %6s %7s %5s %4s %3s' % ('(cin, cout, k, B, N)', 'R', 'U', 'ups', 'S', 'last', 'pairs', 'LDS', 'ppb', 'nb', 'G')]
    for c in cases:
        p = wgrad_plan(c[3], c[4], c[0], c[1], c[2])
        lines.append('%-22s %2d %5d %4d %4d %5d %6d %7d %5d %4d %3d' % (c, p['R'], p['U'], p['ups'], p['S'], p['last_units'], p['pairs'],
                                                                       p['lds'], p['ppb'], p['nb'], p['G']))
    return '\n'.join(lines)


# ---- train_head.hip ----------------------------------------------------------------------------------------------------------
HEAD_BLOCK, HEAD_MAX_PARTIALS = 256, 1024


def head_plan(B, N):
    """at most 1024 partials of ppb pixels, ppb a multiple of the block of 256 threads"""
    npix = B * N * N
    nb = min(cdiv(npix, HEAD_BLOCK), HEAD_MAX_PARTIALS)
    ppb = up(cdiv(npix, nb), HEAD_BLOCK)
    nb = cdiv(npix, ppb)
    return dict(nb=nb, ppb=ppb, last_pixels=npix - (nb - 1) * ppb, loss_passes=ppb // HEAD_BLOCK, finish_passes=cdiv(nb, HEAD_BLOCK))


def head_workspace_bytes(B, N):
    """one float64 per partial, rounded up to 256 bytes: the size resolves nb to 32 partials only"""
    return up(head_plan(B, N)['nb'] * 8, 256)


# (B, N, C)
HEAD_REGIMES = {
    (257, 16, 2): dict(nb=257, ppb=256, finish_passes=2),
    (5, 128, 2): dict(nb=320, ppb=256, finish_passes=2),
    (1025, 16, 2): dict(nb=513, ppb=512, last_pixels=256, loss_passes=2, finish_passes=3),
    (1025, 16, 8): dict(nb=513, ppb=512, last_pixels=256, loss_passes=2, finish_passes=3),
}


# ---- ann_train.hip -----------------------------------------------------------------------------------------------------------
ANN_LDS_FLOATS, ANN_ROWS, ANN_PAD, ANN_MAX_PARTS = 15000, 128, 4, 256


def ann_tile_rows(s, hidden):
    """rows of a full tile: one LDS column per input, activation, delta and one of ones, each of RT + 4 floats, RT a multiple
    of four and at most 128"""
    widths = [s * s] + list(hidden) + [1]
    cols = sum(widths[:-1]) + sum(widths[1:]) + 1
    return min(ANN_ROWS, (ANN_LDS_FLOATS // cols) // 4 * 4 - ANN_PAD)


def ann_plan(s, hidden, n):
    """tiles of a batch of n rows, workgroups, the most tiles one workgroup walks, rows of the last tile"""
    RT = ann_tile_rows(s, hidden)
    tiles = cdiv(n, RT)
    nparts = min(tiles, ANN_MAX_PARTS)
    return dict(RT=RT, tiles=tiles, nparts=nparts, tiles_per_workgroup=cdiv(tiles, nparts), last_rows=n - (tiles - 1) * RT)
