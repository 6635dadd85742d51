"""Test support for the dense dispatch paths (Linear, GRU cell, weight gradient): a plain-Python restatement of the three
host dispatches, float64 references of every dense operation, and case builders that put row counts and widths exactly
at the places where the kernels switch paths.  Never imported by the product package.

Constants (copied here with their source; tests/test_dense_paths_cpu.py checks their arithmetic):
  * K_LDS_BUDGET = 160 KiB            ptgnn_amd/csrc/stream_gemm.hip:61   kLdsBudget
  * K_EPI_BYTES = 16 + 8*8*36*4       ptgnn_amd/csrc/stream_gemm.hip:62   kEpiBytes (unit counter + 8 transposing slabs)
  * K_TQ_LD = 36, K_TQ_FLOATS = 288   ptgnn_amd/csrc/stream_gemm.hip:237-238  kTqLd, kTqFloats
  * slab_bytes(K, rows)               ptgnn_amd/csrc/stream_gemm.hip:133  Slab::bytes = rows * (K + 4) * 4
  * K_RING_PANEL = 64, K_RING_LD = 68 ptgnn_amd/csrc/stream_gemm.hip:640-641
  * K_RING_PANEL_FLOATS = 96 * 68     ptgnn_amd/csrc/stream_gemm.hip:642  (GRU ring: 3 x 32 gate rows per panel)
  * K_RING_WAVES = 4                  ptgnn_amd/csrc/stream_gemm.hip:643
  * K_LIN_RING_PANEL_FLOATS = 128*68  ptgnn_amd/csrc/stream_gemm.hip:763
  * RING_MIN_ROWS = 32 * 64 = 2048    ptgnn_amd/csrc/stream_gemm.hip:1390 (`rows >= 32 * 64 || forced`)
  * UNITS_PER_CU = 8 * 3 = 24         ptgnn_amd/csrc/stream_gemm.hip:1396 (`units < CUs * 8 * 3`)
  * MAX_SLABS = 4                     ptgnn_amd/csrc/stream_gemm.hip:1396 (`(n_out + bn - 1) / bn > 4`)
  * K_NUM_XCD = 8                     ptgnn_amd/csrc/common.h:43          (dense_runs, stream_gemm.hip:1328)
  * GRU_SLAB_ROWS = 96                ptgnn_amd/csrc/stream_gemm.hip:1443 (`Slab::bytes(K, 96)`)
  * blocks_for(width)                 ptgnn_amd/csrc/wgrad_stream.hip:407
  * K_WGRAD_WAVES = 4                 ptgnn_amd/csrc/wgrad_stream.hip:36  kWavesPerWg
  * WGRAD_MIN_CH = 64                 ptgnn_amd/csrc/wgrad_stream.hip:450 (rows per wave, at least)
  * K_WGRAD_PER_CU = 3, TILE_MIN_CH = 256   ptgnn_amd/csrc/edge_wgrad.hip:265, :279 (tile form: rows per chunk, at least)
  * WGRAD_STEP = 32                   ptgnn_amd/csrc/edge_wgrad.hip:33    PTGNN_WGRAD_STEP (rows per LDS stage)
  * GATES_BWD_MAX_BLOCKS = 65536      ptgnn_amd/csrc/dense_f32.hip:520    (256 threads, one float4 each, grid-stride)
  * the tile Linear picks 128 x 64 tiles for n_out <= 128, else 128 x 128: ptgnn_amd/csrc/dense_f32.hip:413
"""
from collections import namedtuple

import torch

K_LDS_BUDGET = 160 * 1024
K_EPI_BYTES = 16 + 8 * 8 * 36 * 4
K_TQ_LD = 36
K_TQ_FLOATS = 8 * K_TQ_LD
K_RING_PANEL = 64
K_RING_LD = K_RING_PANEL + 4
K_RING_PANEL_FLOATS = 96 * K_RING_LD
K_RING_WAVES = 4
K_LIN_RING_PANEL_FLOATS = 128 * K_RING_LD
RING_MIN_ROWS = 32 * 64
UNITS_PER_CU = 8 * 3
MAX_SLABS = 4
K_NUM_XCD = 8
GRU_SLAB_ROWS = 96
K_WGRAD_WAVES = 4
WGRAD_MIN_CH = 64
K_WGRAD_PER_CU = 3
TILE_MIN_CH = 256
WGRAD_STEP = 32
GATES_BWD_MAX_BLOCKS = 65536

TOL = 1e-5          # BASELINE north star: forward values, scaled by max(1, |want|inf)
GRAD_TOL = 2e-5     # gradients, scaled the same way (tests/test_gpu_parity.py dense autograd test)
EPS32 = 2.0 ** -24  # one fp32 rounding, relative

FORCE, LIN_RING, LIN_BN, GRU_RING = ("PTGNN_AMD_FORCE_STREAM", "PTGNN_AMD_LINEAR_RING", "PTGNN_AMD_LINEAR_BN",
                                     "PTGNN_AMD_GRU_RING")
ENV_SWITCHES = (FORCE, LIN_RING, LIN_BN, GRU_RING)     # re-read by the library on every call


def slab_bytes(k, rows):
    return rows * (k + 4) * 4


def resident_lds(k, rows):
    """Dynamic LDS of a resident-slab launch (stream_gemm.hip:1399, :1444): slab + counter + 8 transposing slabs."""
    return slab_bytes(k, rows) + 16 + 8 * K_TQ_FLOATS * 4


def dense_runs(nrb, ncs, max_wg):
    """stream_gemm.hip:1328 dense_runs -> (runs per slab, run length in 32-row units)."""
    rps = max(max_wg // ncs, 1)
    if rps >= K_NUM_XCD and (rps // K_NUM_XCD * K_NUM_XCD) * ncs * 10 >= max_wg * 9:
        rps = rps // K_NUM_XCD * K_NUM_XCD
    rps = min(rps, nrb)
    run_len = (nrb + rps - 1) // rps
    return (nrb + run_len - 1) // run_len, run_len


# ---------------------------------------------------------------------------------------------------------------------
# the three host dispatches
# ---------------------------------------------------------------------------------------------------------------------
Route = namedtuple("Route", "name vec_store slabs")

LINEAR_ROUTES = ("tile_nj1", "tile_nj2", "resident_nb1", "resident_nb2", "resident_nb3", "resident_nb4",
                 "resident_bn64", "ring")
GRU_ROUTES = ("gru_tile_aligned", "gru_tile_unaligned", "gru_resident", "gru_ring")
WGRAD_ROUTES = tuple(f"wgrad_stream_{a}x{b}" for a in (1, 2, 4) for b in (1, 2, 4)) + ("wgrad_tile",)
ALL_ROUTES = LINEAR_ROUTES + GRU_ROUTES + WGRAD_ROUTES

# the launch counter (ops.launch_counts) every route name must move by exactly one
DENSE_COUNTERS = ("k_stream_linear", "k_stream_linear_ring", "k_linear_tlp", "k_stream_gru", "k_stream_gru_ring",
                  "k_gru", "k_wgrad_stream", "k_edge_wgrad")


def counter_of(name):
    if name.startswith("tile_nj"):
        return "k_linear_tlp"
    if name.startswith("resident_"):
        return "k_stream_linear"
    return {"ring": "k_stream_linear_ring", "gru_tile_aligned": "k_gru", "gru_tile_unaligned": "k_gru",
            "gru_resident": "k_stream_gru", "gru_ring": "k_stream_gru_ring", "wgrad_tile": "k_edge_wgrad"}.get(
                name, "k_wgrad_stream")


def linear_route(rows, k, n_out, ld_x=None, ld_y=None, aligned=True, addend=False, env=None, cus=256, mode=1,
                 y_aligned=True, ld_add=None, add_aligned=True):
    """ptgnn_amd_linear_f32 / ptgnn_amd_linear_add_f32 (dense_f32.hip:401, :443) over stream_linear
    (stream_gemm.hip:1361).  `aligned`: x (and the weight) start on 16 bytes; `y_aligned` / `add_aligned` the same for
    the output / the addend.  `mode` 0 = ops.set_gemm_mode("tile").  Returns Route(name, vec_store, column slabs);
    name None = no launch (rows == 0), "unsupported" = linear_add answers EUNSUPPORTED (the host then runs the plain
    Linear and adds)."""
    env = env or {}
    ld_x = k if ld_x is None else ld_x
    ld_y = n_out if ld_y is None else ld_y
    ld_add = n_out if ld_add is None else ld_add
    vec = 1 if (ld_y % 4 == 0 and y_aligned) else 0
    if rows == 0:
        return Route(None, vec, 0)

    def tile():
        if addend:
            return Route("unsupported", vec, 0)
        nj = 1 if n_out <= 128 else 2                       # dense_f32.hip:413
        return Route(f"tile_nj{nj}", vec, (n_out + 64 * nj - 1) // (64 * nj))

    if mode == 0:
        return tile()
    if addend and (not vec or ld_add % 4 != 0 or not add_aligned):      # :1367
        return tile()
    if k % 64 != 0 or n_out % 32 != 0 or ld_x % 4 != 0 or not aligned:   # :1368
        return tile()
    bn = 128 if n_out >= 128 else n_out
    fits128 = slab_bytes(k, 128) + K_EPI_BYTES <= K_LDS_BUDGET
    fits64 = slab_bytes(k, 64) + K_EPI_BYTES <= K_LDS_BUDGET
    want = int(env.get(LIN_BN, "0") or 0)
    ring_env = env.get(LIN_RING)
    force_ring = bool(ring_env) and ring_env[0] == "1"
    no_ring = bool(ring_env) and ring_env[0] == "0"
    forced = env.get(FORCE, "")[:1] == "1"
    if (not force_ring and n_out % 128 == 0 and n_out <= 256 and fits64
            and (want == 64 or (want != 128 and not fits128))):          # :1383
        bn = 64
    ncs = (n_out + bn - 1) // bn
    ring_shape = n_out % 128 == 0 and n_out * k < (1 << 30) and (rows >= RING_MIN_ROWS or forced)
    ring = ring_shape and (force_ring or (not no_ring and slab_bytes(k, bn) + K_EPI_BYTES > K_LDS_BUDGET))
    if ring:
        return Route("ring", vec, ncs)
    units = (rows + 31) // 32 * ncs
    if not forced and (units < cus * UNITS_PER_CU or ncs > MAX_SLABS):   # :1396
        return tile()
    if resident_lds(k, bn) > K_LDS_BUDGET:                               # :1417
        return tile()
    if bn == 64 and n_out >= 128:
        return Route("resident_bn64", vec, ncs)
    return Route(f"resident_nb{bn // 32}", vec, ncs)


def gru_route(n, m, hd, ld_a=None, ld_h=None, ld_out=None, aligned=True, env=None, mode=1):
    """gru_launch (dense_f32.hip:461) over stream_gru (stream_gemm.hip:1433).  No size floor: the GRU streams at every
    row count.  Returns a GRU_ROUTES name, or None for n == 0 (no launch)."""
    env = env or {}
    ld_a = m if ld_a is None else ld_a
    ld_h = hd if ld_h is None else ld_h
    ld_out = hd if ld_out is None else ld_out
    if n == 0:
        return None
    tile = ("gru_tile_aligned" if (m % 4 == 0 and hd % 4 == 0 and ld_a % 4 == 0 and ld_h % 4 == 0 and aligned)
            else "gru_tile_unaligned")                                   # dense_f32.hip:478
    if mode == 0:
        return tile
    if m % 64 != 0 or hd % 64 != 0 or ld_a % 4 != 0 or ld_h % 4 != 0 or ld_out % 4 != 0 or not aligned:   # :1438
        return tile
    lds = resident_lds(m + hd, GRU_SLAB_ROWS)
    ring_env = env.get(GRU_RING)
    force_ring = bool(ring_env) and ring_env[0] == "1"
    no_ring = bool(ring_env) and ring_env[0] == "0"
    if (lds > K_LDS_BUDGET and not no_ring) or force_ring:               # :1452
        return "gru_ring"
    if lds > K_LDS_BUDGET:                                               # :1463
        return tile
    return "gru_resident"


def blocks_for(width):
    """wgrad_stream.hip:407: 32-column blocks per side of the streaming weight-gradient tile (0 = not its shape)."""
    return 4 if width % 128 == 0 else (2 if width % 64 == 0 else (1 if width % 32 == 0 else 0))


def wgrad_route(rows, k, n_out):
    """weight_grad_launch (edge_wgrad.hip:299) in its dense form over stream_wgrad (wgrad_stream.hip:423), for a
    process that did not set PTGNN_AMD_WGRAD_STREAM=0.  grad_w is [n_out, k]: side A = n_out, side B = k.  None for
    rows == 0 (the Python wrapper returns zeros without a launch)."""
    if rows == 0:
        return None
    if k % 4 != 0 or n_out % 4 != 0:
        return "unsupported"                                             # edge_wgrad.hip:306 (dense.py pads to 4)
    nba, nbb = blocks_for(n_out), blocks_for(k)
    if nba == 0 or nbb == 0:
        return "wgrad_tile"
    return f"wgrad_stream_{nba}x{nbb}"


def wgrad_rows_per_workgroup(rows, k, n_out, cus):
    """Rows one workgroup of the taken weight-gradient kernel reduces: the streaming form gives each of its 4 waves
    `ch` rows (wgrad_stream.hip:445-450), the tile form one chunk of chunk_edges_for rows (edge_wgrad.hip:266)."""
    route = wgrad_route(rows, k, n_out)
    if route == "wgrad_tile":
        tiles = ((n_out + 127) // 128) * ((k + 127) // 128)
        slots, rounds = K_WGRAD_PER_CU * cus, 1
        while True:
            budget = max(slots * rounds // tiles - 1, 1)
            ch = (rows + budget - 1) // budget
            if ch <= 8192 or rounds >= 64:
                break
            rounds += 1
        return max((ch + WGRAD_STEP - 1) // WGRAD_STEP * WGRAD_STEP, TILE_MIN_CH)
    nba, nbb = blocks_for(n_out), blocks_for(k)
    tiles = (n_out // (32 * nba)) * (k // (32 * nbb))
    budget = max(cus // tiles - 1, 1)
    ch = (rows + K_WGRAD_WAVES * budget - 1) // (K_WGRAD_WAVES * budget)
    ch = max((ch + 1) & ~1, WGRAD_MIN_CH)
    return K_WGRAD_WAVES * ch


# ---------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------
def _act64(v, act):
    return torch.tanh(v) if act == "tanh" else (torch.relu(v) if act == "relu" else v)


def _d(t):
    return None if t is None else t.detach().double().cpu()


def linear_ref(x, w, b=None, act=None, addend=None):
    """act(x W^T + b) + addend in float64 (weight in nn.Linear layout [n_out, k])."""
    x, w, b, addend = _d(x), _d(w), _d(b), _d(addend)
    y = x @ w.t()
    if b is not None:
        y = y + b
    y = _act64(y, act)
    return y if addend is None else y + addend


def gru_ref(a, h, w_ih, w_hh, b_ih=None, b_hh=None):
    """nn.GRUCell in float64, written out: (h', r, z, n, gh_n) with gh_n = (h W_hn^T + b_hn), the term r multiplies."""
    a, h, w_ih, w_hh, b_ih, b_hh = (_d(t) for t in (a, h, w_ih, w_hh, b_ih, b_hh))
    hd = h.shape[1]
    gi, gh = a @ w_ih.t(), h @ w_hh.t()
    if b_ih is not None:
        gi, gh = gi + b_ih, gh + b_hh
    r = torch.sigmoid(gi[:, :hd] + gh[:, :hd])
    z = torch.sigmoid(gi[:, hd:2 * hd] + gh[:, hd:2 * hd])
    gh_n = gh[:, 2 * hd:]
    n = torch.tanh(gi[:, 2 * hd:] + r * gh_n)
    return (1.0 - z) * n + z * h, r, z, n, gh_n


def gates_backward_ref(grad_out, gates, h, device="cpu"):
    """(d_gi, d_gh, d_h) of the GRU gate math by torch float64 autograd over the restatement above.  `gates` =
    r | z | n | gh_n [rows, 4 hd] as ops.gru_cell_train returns them; the pre-activations autograd differentiates are
    rebuilt from them (logit(r), logit(z), atanh(n) - r gh_n), h enters directly (its direct term g z only)."""
    g, gates, h = (t.detach().to(device=device, dtype=torch.float64) for t in (grad_out, gates, h))
    hd = h.shape[1]
    r0, z0, n0, ghn0 = (gates[:, i * hd:(i + 1) * hd] for i in range(4))
    s_r = torch.logit(r0).requires_grad_(True)          # i_r + h_r: both halves receive its gradient
    s_z = torch.logit(z0).requires_grad_(True)
    h_n = ghn0.clone().requires_grad_(True)
    i_n = (torch.atanh(n0) - r0 * ghn0).requires_grad_(True)
    hh = h.clone().requires_grad_(True)
    r, z = torch.sigmoid(s_r), torch.sigmoid(s_z)
    out = (1.0 - z) * torch.tanh(i_n + r * h_n) + z * hh
    d_sr, d_sz, d_in, d_hn, d_h = torch.autograd.grad(out, [s_r, s_z, i_n, h_n, hh], g)
    return torch.cat([d_sr, d_sz, d_in], 1), torch.cat([d_sr, d_sz, d_hn], 1), d_h


def gates_backward_scale(grad_out, gates, h, device="cpu"):
    """The magnitudes S the derived bound of the gate-math backward multiplies: the kernel's formulas
    (dense_f32.hip:348-358) in float64 on absolute values with (1 - z) -> 1, (1 - n^2) -> 1, (h - n) -> |h| + |n|.
    Same layout as `gates_backward_ref`."""
    g, gates, h = (t.detach().to(device=device, dtype=torch.float64).abs() for t in (grad_out, gates, h))
    hd = h.shape[1]
    r, z, n, ghn = (gates[:, i * hd:(i + 1) * hd] for i in range(4))
    s_n = g
    s_r = g * ghn * r * (1.0 - r).abs()
    s_z = g * (h + n) * z * (1.0 - z).abs()
    return torch.cat([s_r, s_z, s_n], 1), torch.cat([s_r, s_z, g * r], 1), g * z


def act_dropout_backward_ref(grad, y, keep, scale, act):
    """d/du of keep * scale * act(u) by torch float64 autograd, u rebuilt from y = act(u) (atanh for tanh; relu and
    none: u = y, so y == 0 under relu has gradient 0, as torch gives)."""
    g, y = _d(grad), _d(y)
    u = (torch.atanh(y) if act == "tanh" else y.clone()).requires_grad_(True)
    out = _act64(u, act)
    if keep is not None:
        out = out * keep.detach().cpu().double() * float(scale)
    (d_u,) = torch.autograd.grad(out, [u], g)
    return d_u


def act_dropout_backward_scale(grad, keep, scale):
    """|grad| * |keep * scale| with (1 - y^2) -> 1."""
    s = _d(grad).abs()
    return s if keep is None else s * keep.detach().cpu().double() * abs(float(scale))


def weight_grad_ref(x, grad_y):
    """(grad_w [n_out, k], grad_b [n_out]) in float64."""
    x, gy = _d(x), _d(grad_y)
    return gy.t() @ x, gy.sum(0)


# ---------------------------------------------------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------------------------------------------------
ROW_TAILS = (1, 31, 32, 33, 127, 128, 129, 2047, 2048, 2049)


def ragged_run_rows(cus, ncs=1, ring=False):
    """The smallest row count whose 32-row units do not divide into equal runs: ceil(rows / 32) is not a multiple of
    the run length dense_runs gives one workgroup, and the last unit is ragged too."""
    max_wg = 2 * cus if ring else cus
    nrb = max_wg // ncs + 1
    while True:
        _, run_len = dense_runs(nrb, ncs, max_wg)
        if run_len > 1 and nrb % run_len != 0:
            return nrb * 32 - 5
        nrb += 1


def row_counts(cus, ncs=1, ring=False):
    return ROW_TAILS + (ragged_run_rows(cus, ncs, ring),)


def identity_probe(k, rows, offset=0):
    """x [rows, k] = zero rows around I_K at row `offset`: without a bias y[offset : offset + k] must be W^T bit for
    bit on every route (products with 1.0 and sums with 0.0 are exact) and every other row exactly zero."""
    assert rows >= offset + k
    x = torch.zeros(rows, k)
    x[offset:offset + k] = torch.eye(k)
    return x


def linear_case(rows, k, n_out, seed=0, bias=True):
    g = torch.Generator().manual_seed(1000 * k + n_out + 7 * rows + seed)
    x = torch.randn(rows, k, generator=g)
    w = torch.randn(n_out, k, generator=g) / k ** 0.5
    b = torch.randn(n_out, generator=g) if bias else None
    return x, w, b


def gru_case(n, m, hd, seed=0):
    g = torch.Generator().manual_seed(1000 * m + hd + 7 * n + seed)
    a, h = torch.randn(n, m, generator=g), torch.randn(n, hd, generator=g)
    w_ih, w_hh = torch.randn(3 * hd, m, generator=g) / m ** 0.5, torch.randn(3 * hd, hd, generator=g) / hd ** 0.5
    b_ih, b_hh = torch.randn(3 * hd, generator=g) * 0.1, torch.randn(3 * hd, generator=g) * 0.1
    return a, h, w_ih, w_hh, b_ih, b_hh


# (k, n_out, env, mode): every Linear shape of the GPU matrix with the switches that route it.  FORCE lifts the size
# floors so the row tails reach the streaming kernels; the real floors have their own test.
_F = {FORCE: "1"}
LINEAR_SHAPES = (
    # tile kernels by mode, 128 x 64 and 128 x 128 tiles
    (64, 128, {}, 0), (128, 96, {}, 0), (256, 160, {}, 0), (64, 544, {}, 0),
    # tile-only shapes in streaming mode: k % 4 != 0, n_out 129 / 130
    (130, 70, _F, 1), (64, 129, _F, 1), (128, 130, _F, 1),
    # resident slab, one to four 32-column blocks; ragged last slabs at n_out 160 / 224 / 288
    (64, 32, _F, 1), (768, 32, _F, 1), (128, 64, _F, 1), (576, 64, _F, 1), (256, 96, _F, 1), (320, 96, _F, 1),
    (64, 128, _F, 1), (256, 128, _F, 1), (128, 160, _F, 1), (256, 224, _F, 1), (128, 256, _F, 1), (64, 288, _F, 1),
    (128, 384, _F, 1), (64, 512, _F, 1), (64, 544, _F, 1),
    # 64-column slabs: K = 320 .. 576 at n_out 128 / 256
    (320, 128, _F, 1), (576, 128, _F, 1), (576, 256, _F, 1), (128, 128, {FORCE: "1", LIN_BN: "64"}, 1),
    # panel ring: K beyond the slabs, n_out beyond 256 at K = 320, forced where the slab fits
    (640, 128, _F, 1), (768, 256, _F, 1), (320, 384, _F, 1), (768, 512, _F, 1), (128, 128, {FORCE: "1", LIN_RING: "1"}, 1),
    # nothing fits and the shape is no ring shape: back to the tile kernel
    (640, 96, _F, 1), (768, 160, _F, 1),
)

GRU_SHAPES = ((64, 64), (128, 128), (64, 320), (128, 256), (192, 256), (256, 256), (384, 128), (24, 16), (100, 36),
              (130, 70))

WGRAD_STREAM_WIDTHS = (32, 64, 96, 128, 160, 384)
WGRAD_TILE_WIDTHS = (36, 100, 132)
