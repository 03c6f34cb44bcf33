"""Host logic of the weight packs (lighthand_amd/weight_packs.py): the early / late split of the tiled pack launch and the work-item tables
of the two pack kernels, as pure functions of the layer sizes; and ``pack_image_ref``, the host reference of a pack image that the GPU
tests of the pack kernels compare against, checked here against the framework's convolutions.  No GPU, no kernel library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lighthand_amd.weight_packs import late_pack_split, pack_chunk_table, pack_tile_table


def pack_image_ref(w, n_out, n_in, strides, taps_rs, dtype):
    """The pack image [n_out padded to 128][tap][n_in padded to the 128-byte step] of the fp32 tensor ``w`` (read as flat memory), by plain
    indexing on the CPU: img[o][t][k] = w.flatten()[o*so + k*si + r_t*sr + s_t*ss] for o < n_out and k < n_in, zero elsewhere, then
    one ``Tensor.to(dtype)`` (round to nearest even)."""
    assert w.dtype == torch.float32 and w.is_contiguous() and len(taps_rs) > 0
    so, si, sr, ss = strides
    kstep = 128 // torch.empty((), dtype=dtype).element_size()
    rows, kpad = -(-n_out // 128) * 128, -(-n_in // kstep) * kstep
    o = torch.arange(n_out).view(-1, 1, 1)
    t = torch.tensor([r * sr + s * ss for r, s in taps_rs]).view(1, -1, 1)
    k = torch.arange(n_in).view(1, 1, -1)
    img = torch.zeros(rows, len(taps_rs), kpad, dtype=torch.float32)
    img[:n_out, :, :n_in] = w.detach().cpu().flatten()[o * so + k * si + t]
    return img.to(dtype)


def phase_taps(k, p, s):
    """The tap subsets of the s x s sub-pixel phases of a k x k kernel with padding p, as engine.py forms them for a transposed
    convolution (and for the data gradient of a stride-s convolution): per phase (ph, pw) the taps (r, q) with (ph + p - r) and
    (pw + p - q) divisible by s, and the input displacement ((ph + p - r) / s, (pw + p - q) / s) of each."""
    out = []
    for ph in range(s):
        for pw in range(s):
            sub = [(r, q) for r in range(k) for q in range(k) if (ph + p - r) % s == 0 and (pw + p - q) % s == 0]
            out.append((ph, pw, sub, [((ph + p - r) // s, (pw + p - q) // s) for r, q in sub]))
    return out


def _gemm(img, x, disp, ho, wo):
    """sum_{t,k} img[o][t][k] * x[k][y + dy_t][x + dx_t] in fp64, x read as zero outside its frame and in the channels the image pads."""
    rows, ntaps, kpad = img.shape
    cin, h, w = x.shape
    m = max(max(abs(a), abs(b)) for a, b in disp) + max(ho, wo)
    xp = torch.zeros(kpad, h + 2 * m, w + 2 * m, dtype=torch.float64)
    xp[:cin, m:m + h, m:m + w] = x
    out = torch.zeros(rows, ho, wo, dtype=torch.float64)
    for t, (dy, dx) in enumerate(disp):
        out += torch.einsum("ok,kyx->oyx", img[:, t].double(), xp[:, m + dy:m + dy + ho, m + dx:m + dx + wo])
    return out


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_reference_image_is_the_gemm_operand_of_conv2d():
    """OIHW strides and all taps, as engine.py packs a Conv2d: the fp32 reference image times the shifted input is F.conv2d."""
    cout, cin, k, p, h, w = 6, 5, 3, 1, 4, 7
    g = torch.Generator().manual_seed(3)
    wt = torch.randn(cout, cin, k, k, generator=g)
    x = torch.randn(cin, h, w, generator=g, dtype=torch.float64)
    taps = [(r, q) for r in range(k) for q in range(k)]
    img = pack_image_ref(wt, cout, cin, (cin * k * k, k * k, k, 1), taps, torch.float32)
    assert img.shape == (128, 9, 32)
    got = _gemm(img, x, [(r - p, q - p) for r, q in taps], h, w)
    want = F.conv2d(x[None], wt.double(), padding=p)[0]
    assert _rel(got[:cout], want) < 1e-12
    assert not got[cout:].any()                                                # padded rows are zero rows of the operand
    # the data-gradient pack of the same tensor (transposed strides): the image of conv_transpose2d at stride 1
    dimg = pack_image_ref(wt, cin, cout, (k * k, cin * k * k, k, 1), taps, torch.float32)
    dy = torch.randn(cout, h, w, generator=g, dtype=torch.float64)
    got = _gemm(dimg, dy, [(p - r, p - q) for r, q in taps], h, w)
    want = F.conv_transpose2d(dy[None], wt.double(), padding=p)[0]
    assert _rel(got[:cin], want) < 1e-12


def test_reference_image_is_the_gemm_operand_of_conv_transpose2d():
    """[C_in][C_out][4][4] with the strides and the four phase tap subsets of engine.py's deconv packs: phase (ph, pw) of the
    reference image produces the output pixels (2a + ph, 2b + pw) of F.conv_transpose2d(stride 2, padding 1); the 16-tap
    data-gradient pack of the same tensor is the stride-2 convolution of the output gradient."""
    cin, cout, k, p, h, w = 5, 6, 4, 1, 3, 4
    g = torch.Generator().manual_seed(4)
    wt = torch.randn(cin, cout, k, k, generator=g)
    x = torch.randn(cin, h, w, generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(x[None], wt.double(), stride=2, padding=p)[0]
    assert want.shape == (cout, 2 * h, 2 * w)
    seen = []
    for ph, pw, sub, disp in phase_taps(k, p, 2):
        assert len(sub) == 4
        seen += sub
        img = pack_image_ref(wt, cout, cin, (k * k, cout * k * k, k, 1), sub, torch.float32)
        got = _gemm(img, x, disp, h, w)
        assert _rel(got[:cout], want[:, ph::2, pw::2]) < 1e-12, (ph, pw)
    assert sorted(seen) == [(r, q) for r in range(k) for q in range(k)]        # the phases split the taps
    taps = [(r, q) for r in range(k) for q in range(k)]
    dimg = pack_image_ref(wt, cin, cout, (cout * k * k, k * k, k, 1), taps, torch.float32)
    dy = torch.randn(cout, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    full = _gemm(dimg, dy, [(r - p, q - p) for r, q in taps], 2 * h, 2 * w)[:cin, ::2, ::2]
    assert _rel(full, F.conv2d(dy[None], wt.double(), stride=2, padding=p)[0]) < 1e-12


def test_reference_image_pads_and_rounds():
    """Row and K padding per element size, the stem's staged layout (one tap per kernel row, tap stride 0 along s), and one rounding."""
    w = torch.arange(64 * 7 * 32, dtype=torch.float32).view(64, 7, 8, 4)
    taps = [(r, 0) for r in range(7)]
    for dt, kpad in ((torch.float32, 32), (torch.bfloat16, 64), (torch.float16, 64)):
        img = pack_image_ref(w, 64, 32, (7 * 32, 1, 32, 0), taps, dt)
        assert img.shape == (128, 7, kpad) and img.dtype == dt
        assert torch.equal(img[:64, :, :32].float(), w.view(64, 7, 32).to(dt).float())
        assert not img[64:].float().any() and not img[:, :, 32:].float().any()
    tie = torch.tensor([0x3F808000, 0x3F818000], dtype=torch.int32).view(torch.float32)      # halfway between two bf16 values
    got = pack_image_ref(tie, 1, 2, (0, 1, 0, 0), [(0, 0)], torch.bfloat16)[0, 0, :2].view(torch.int16).tolist()
    assert got == [0x3F80, 0x3F82]                                                            # to the even neighbour, down and up


@pytest.mark.parametrize("sizes,want", [
    ([7] * 15, None),                       # fewer than 16 convolutions
    ([1] * 20, None),                       # the tail of <= 0.8 of the total starts at conv 4: fewer than 8 layers in front of it
    ([1] * 12 + [10] * 8, (13, 5)),         # total 92: seven 10s (70 <= 73.6) are late; fork 13 - max(8, int(0.35 * 20)) = 5
    ([1] * 8 + [100] * 8, (10, 2)),         # total 808: six 100s (600 <= 646.4) are late; fork 10 - max(8, int(0.35 * 16)) = 2
    ([1] * 19 + [100], None),               # the last layer alone exceeds 0.8 of the total: nothing can be late
])
def test_late_pack_split_follows_the_rule(sizes, want):
    assert late_pack_split(sizes) == want


def test_tile_table_is_row_major_per_conv():
    dims = [(33, 64), (32, 31)]
    want = [(0, a, b) for a in range(2) for b in range(2)] + [(1, 0, 0)]         # ceil(33/32) * ceil(64/32) = 4 tiles, then 1 * 1
    assert pack_tile_table(dims) == want
    for i, (d0, d1) in enumerate(dims):
        assert sum(1 for t in want if t[0] == i) == -(-d0 // 32) * -(-d1 // 32)


@pytest.mark.parametrize("chunk", [1, 1000, 4096, 1 << 20])
@pytest.mark.parametrize("kstep", [32, 64])
def test_chunk_table_covers_every_padded_element_once(chunk, kstep):
    items = [(70, 33, 9), (128, 64, 1), (1, 1, 1), (129, 65, 4)]               # (n_out, n_in, ntaps)
    if chunk == 1:
        items = items[2:3]                                                     # one chunk per element: the smallest image is enough
    table = pack_chunk_table(items, chunk, kstep)
    assert [i for i, _ in table] == sorted(i for i, _ in table)                # grouped by item, in order
    for i, (n_out, n_in, ntaps) in enumerate(items):
        total = -(-n_out // 128) * 128 * ntaps * -(-n_in // kstep) * kstep
        hits = np.zeros(total, dtype=np.int32)
        for _, s0 in (t for t in table if t[0] == i):
            assert 0 <= s0 < total
            hits[s0:s0 + chunk] += 1                                           # a work item packs [start, min(start + chunk, total))
        assert (hits == 1).all()
