"""Test-side restatement of the discriminator's stride-2 convolution of include/qgx_dconv_train.h, in float64 numpy and in the
ABI's layout: x (B, N, N, C8(cin)), y (B, N/2, N/2, C8(cout)) with zero pad channels, weights (cout, cin, 4, 4), zero padding 1.

  forward(x, w)                    y[b, co, i, j] = sum x[b, ci, 2i - 1 + ky, 2j - 1 + kx] w[co, ci, ky, kx]
  backward_data(dy, w, N)          dx[b, ci, r, s] = sum over r = 2i - 1 + ky, s = 2j - 1 + kx of dy[b, co, i, j] w[co, ci, ky, kx]
  backward_data_by_parity          the same as four 2 x 2-tap convolutions over dy, the way csrc/dconv_train.hip computes it
  backward_weight(x, dy, cin, cout)  dw[co, ci, ky, kx] = sum dy[b, co, i, j] x[b, ci, 2i - 1 + ky, 2j - 1 + kx]

and of the weight gradient's host-side plan (dwgrad_plan, workspace_bytes), a function of the shape alone, as
tests/train_plan_restatement.py does for conv_train.hip.  tests/test_dconv_train_cpu.py pins the operations to torch CPU autograd
of F.conv2d(stride=2, padding=1) and the plan to the library.  A plain helper module.
"""
import numpy as np

from conv_train_restatement import c8, to_layout, from_layout


def _padded(a):
    """planar (B, C, N, N) -> (B, C, N + 2, N + 2) with a zero rim"""
    return np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)))


def forward(x, w):
    w = np.asarray(w, np.float64)
    cout, cin = w.shape[:2]
    xp = _padded(from_layout(np.asarray(x, np.float64), cin))
    No = x.shape[1] // 2
    y = np.zeros((x.shape[0], cout, No, No))
    for ky in range(4):
        for kx in range(4):
            y += np.einsum('oc,bcij->boij', w[:, :, ky, kx], xp[:, :, ky:ky + 2 * No:2, kx:kx + 2 * No:2], optimize=True)
    return to_layout(y)


def backward_data(dy, w, N):
    """the definition, tap by tap: the scatter of every output pixel's gradient onto the 16 input pixels it read"""
    w = np.asarray(w, np.float64)
    cout, cin = w.shape[:2]
    g = from_layout(np.asarray(dy, np.float64), cout)
    No = N // 2
    dxp = np.zeros((g.shape[0], cin, N + 2, N + 2))
    for ky in range(4):
        for kx in range(4):
            dxp[:, :, ky:ky + 2 * No:2, kx:kx + 2 * No:2] += np.einsum('oc,boij->bcij', w[:, :, ky, kx], g, optimize=True)
    return to_layout(dxp[:, :, 1:-1, 1:-1])


def parity_taps(p):
    """row 2i' + p of dx: [(ky, output row offset)] — ky in {1, 3} from rows i', i' - 1 (p = 0), {2, 0} from i', i' + 1 (p = 1)"""
    return [(1, 0), (3, -1)] if p == 0 else [(2, 0), (0, 1)]


def backward_data_by_parity(dy, w, N):
    """four parity classes of a 2 x 2-tap convolution over dy (gathers, no scatter)"""
    w = np.asarray(w, np.float64)
    cout, cin = w.shape[:2]
    g = _padded(from_layout(np.asarray(dy, np.float64), cout))         # output row i is padded row i + 1
    No = N // 2
    dx = np.zeros((g.shape[0], cin, N, N))
    for py in (0, 1):
        for px in (0, 1):
            acc = np.zeros((g.shape[0], cin, No, No))
            for ky, di in parity_taps(py):
                for kx, dj in parity_taps(px):
                    acc += np.einsum('oc,boij->bcij', w[:, :, ky, kx], g[:, :, 1 + di:1 + di + No, 1 + dj:1 + dj + No], optimize=True)
            dx[:, :, py::2, px::2] = acc
    return to_layout(dx)


def backward_weight(x, dy, cin, cout):
    xp = _padded(from_layout(np.asarray(x, np.float64), cin))
    g = from_layout(np.asarray(dy, np.float64), cout)
    No = g.shape[-1]
    dw = np.zeros((cout, cin, 4, 4))
    for ky in range(4):
        for kx in range(4):
            dw[:, :, ky, kx] = np.einsum('boij,bcij->oc', g, xp[:, :, ky:ky + 2 * No:2, kx:kx + 2 * No:2], optimize=True)
    return dw


def case_data(cin, cout, B, N, seed, integer):
    """x, w, dy of one case in the ABI's layout (float32, zero pad channels); integer: drawn from -3 ... 3"""
    rs = np.random.RandomState(seed)
    if integer:
        draw = lambda *s: rs.randint(-3, 4, size=s).astype(np.float32)
    else:
        draw = lambda *s: rs.randn(*s).astype(np.float32)
    x, dy = to_layout(draw(B, cin, N, N)), to_layout(draw(B, cout, N // 2, N // 2))
    return x, draw(cout, cin, 4, 4), dy


# ---- the weight gradient's plan ------------------------------------------------------------------------------------------------
TILE, UNIT, WORKGROUPS = 64, 32, 512


def cdiv(a, b):
    return (a + b - 1) // b


def up(v, m):
    return cdiv(v, m) * m


def dwgrad_plan(B, N, cin, cout):
    """units of 32 output pixels, S shares of `ups` consecutive units, tiles of 64 output channels x 64 (tap, channel) pairs"""
    P = B * (N // 2) ** 2
    U = cdiv(P, UNIT)
    cot_n, nt_n = cdiv(cout, TILE), cdiv(16 * cin, TILE)
    tiles = cot_n * nt_n
    want = min(cdiv(WORKGROUPS, tiles), U)
    ups = cdiv(U, want)
    S = cdiv(U, ups)
    return dict(P=P, U=U, ups=ups, S=S, last_units=U - (S - 1) * ups, last_pixels=P - (U - 1) * UNIT, cot_n=cot_n, nt_n=nt_n,
                tiles=tiles)


def workspace_bytes(B, N, cin, cout):
    """floats, every part rounded up to 64: the packed weights (of the forward, cout x 16 cin8, or of the data gradient,
    16 cin x cout8, whichever is larger) | the shares' slices [S][tiles][64][64]"""
    p = dwgrad_plan(B, N, cin, cout)
    return 4 * (up(max(cout * 16 * c8(cin), 16 * cin * c8(cout)), 64) + up(p['S'] * p['tiles'] * TILE * TILE, 64))


# the GPU cases (cin, cout, B, N) that are there for a regime of the weight gradient, and the regime as data
DCONV_REGIMES = {
    (4, 8, 500, 12): dict(tiles=1, U=563, ups=2, S=282, last_units=1, last_pixels=16),
    (8, 72, 500, 6): dict(cot_n=2, nt_n=2, U=141, ups=2, S=71, last_units=1, last_pixels=20),
    (3, 5, 600, 16): dict(tiles=1, U=1200, ups=3, S=400, last_units=3),
}
