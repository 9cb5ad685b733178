"""fp8 plumbing at kernel level (-m gpu): the conversion every 1-byte image goes through, the amax sites, the weight-image
launch and the delayed-scaling state machine (csrc/operand_images.hip), each against a plain CPU restatement, bit for bit.

 * plb_launch_quantize over every finite bf16 bit pattern and +-inf, the fp32 midpoints between neighbouring fp8 values
   and their neighbours, the saturation edge and subnormals, in both formats: the device's clamp + v_cvt_pk_{fp8,bf8}_f32
   (csrc/common.h: pack_fp8x4) must give torch's OCP bytes (gpu_util.ocp_bytes);
 * plb_launch_amax / plb_launch_quantize_multi: the site's maximum EQUALS max |source| (a maximum of the same values: no
   rounding separates them), padding columns and other sites untouched;
 * plb_launch_fp8_scales / plb_launch_fp8_scales2: a Python model written from the contract in csrc/plbert_kernels.h, driven
   through a dozen calls in the engine's own layout (csrc/engine_fp8.cpp: fp8_update_scales), scale / deq / stats / cleared slots
   equal bit for bit.
NaN inputs are left out: their bytes are not part of the contract."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import F8_SLOTS, F8_STRIDE, assert_fp8_image, fp8_fmax, ptr_array, site_max, stream
from plbert_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SITE = F8_SLOTS * F8_STRIDE


def _all_bf16():
    """Every finite bf16 bit pattern and +-inf (NaN patterns replaced by zero), as [8192, 8] bf16."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    x = bits.clone()
    x[torch.isnan(x)] = 0
    return x.reshape(8192, 8)


def _fp8_values(bf8):
    """All finite non-negative values of the format, ascending (float64)."""
    dt = torch.float8_e5m2 if bf8 else torch.float8_e4m3fn
    v = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(dt).double()
    v = v[torch.isfinite(v) & (v >= 0)]
    return torch.unique(v)


def _fp32_edges(bf8):
    """Midpoints between neighbouring fp8 values, the fp32 values on each side of them, the saturation edge and fp32
    subnormals, both signs, as a flat fp32 tensor."""
    v = _fp8_values(bf8)
    mid = ((v[1:] + v[:-1]) / 2).float()              # <= 5 significant bits: exact in fp32
    assert torch.equal(mid.double(), (v[1:] + v[:-1]) / 2)
    up = torch.nextafter(mid, torch.full_like(mid, float("inf")))
    dn = torch.nextafter(mid, torch.zeros_like(mid))
    mx = fp8_fmax(bf8)
    edge = torch.tensor([mx, mx * (1 + 2.0 ** -5), np.nextafter(np.float32(mx), np.float32(np.inf)), 1e30, float("inf"),
                         1e-45, 1e-40, 2.0 ** -126, 2.0 ** -127, 3e-39, 0.0], dtype=torch.float32)
    x = torch.cat([v.float(), mid, up, dn, edge])
    x = torch.cat([x, -x])
    pad = (-x.numel()) % 8
    return torch.cat([x, torch.zeros(pad)])


def _quantize(L, x, scale, bf8, ld=None, ldo=None, sentinel=0x5A):
    rows, cols = x.shape
    ld, ldo = ld or cols, ldo or cols
    src = torch.zeros(rows, ld, dtype=x.dtype)
    src[:, cols:] = 1e4                                         # values in the gaps must not reach the image
    src[:, :cols] = x
    src = src.to(DEV)
    out = torch.full((rows, ldo), sentinel, dtype=torch.uint8, device=DEV)
    s = torch.tensor([scale], dtype=torch.float32, device=DEV)
    rc = L.plb_launch_quantize(src.data_ptr(), int(x.dtype == torch.bfloat16), rows, cols, ld, s.data_ptr(), out.data_ptr(),
                               ldo, int(bf8), stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu(), s


SCALES = [1.0, float(np.float32(448.0 / 3.7)), 2.0 ** -7, 2.0 ** 9]


@pytest.mark.parametrize("bf8", [0, 1])
@pytest.mark.parametrize("scale", SCALES)
def test_quantize_every_bf16_value(bf8, scale):
    L = _lib.lib()
    x = _all_bf16()
    out, s = _quantize(L, x, scale, bf8)
    assert_fp8_image(out, x, s, bf8, slice(None))


@pytest.mark.parametrize("bf8", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -7, float(np.float32(448.0 / 3.7))])
def test_quantize_fp32_midpoints_saturation_and_subnormals(bf8, scale):
    """At a power-of-two scale the product is exact and the midpoints stay midpoints (the ties of round-to-nearest-even);
    448 / 3.7 moves them off the grid (the product's own rounding then decides)."""
    L = _lib.lib()
    x = _fp32_edges(bf8)
    x = (x / scale if scale != float(np.float32(448.0 / 3.7)) else x).float().reshape(-1, 8)
    out, s = _quantize(L, x, scale, bf8)
    assert_fp8_image(out, x, s, bf8, slice(None))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_quantize_strided_with_sentinel_gaps(dtype):
    L = _lib.lib()
    g = torch.Generator().manual_seed(3)
    rows, cols, ld, ldo = 37, 40, 56, 48
    x = (torch.randn(rows, cols, generator=g) * 3).to(dtype)
    for bf8 in (0, 1):
        out, s = _quantize(L, x, 60.0, bf8, ld=ld, ldo=ldo, sentinel=0xA5)
        assert_fp8_image(out, x, s, bf8, slice(None), sentinel=0xA5, cols=cols)


def test_quantize_grid_stride_loop():
    """More than 2048 blocks x 256 threads x 8 elements: every thread runs the loop more than once."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(4)
    rows, cols = 4100, 1032
    assert rows * cols > 2048 * 256 * 8
    x = (torch.randn(rows, cols, generator=g) * 20).to(torch.bfloat16)
    out, s = _quantize(L, x, 448.0 / 70.0, 0)
    assert_fp8_image(out, x, s, 0, slice(None))
    xf = torch.randn(rows, cols, generator=g) * 1e-3
    out, s = _quantize(L, xf, 2.0 ** 20, 1)
    assert_fp8_image(out, xf, s, 1, slice(None))


# ------------------------------------------------------------------------------------------------------------- amax
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("where", ["first", "last", "negative"])
@pytest.mark.parametrize("prior", [0.0, 0.5, 1e9])
def test_amax_site(dtype, where, prior):
    L = _lib.lib()
    g = torch.Generator().manual_seed(5)
    rows, cols, ld = 301, 48, 64
    x = torch.rand(rows, ld, generator=g) * 2 - 1
    peak = 7.25
    if where == "first":
        x[0, 0] = peak
    elif where == "last":
        x[rows - 1, cols - 1] = peak
    else:
        x[rows // 2, cols // 3] = -peak
    x[:, cols:] = 1e6                                          # padding columns: larger, must not count
    x[rows - 1, cols:] = -1e7
    x = x.to(dtype)
    site = torch.zeros(SITE, dtype=torch.float32)
    site[F8_STRIDE * 37] = prior                              # a value already in the site (atomic-max semantics)
    site = site.to(DEV)
    xd = x.to(DEV)
    rc = L.plb_launch_amax(xd.data_ptr(), int(dtype == torch.bfloat16), rows, cols, ld, site.data_ptr(), stream())
    assert rc == 0
    torch.cuda.synchronize()
    want = max(float(x[:, :cols].float().abs().max()), prior)
    assert want == (peak if prior < peak else prior)
    assert site_max(site) == want
    words = site.cpu().reshape(F8_SLOTS, F8_STRIDE)
    assert bool((words[:, 1:] == 0).all())                      # only the slot words are written


def test_amax_refuses_unaligned_columns():
    L = _lib.lib()
    site = torch.zeros(SITE, device=DEV)
    x = torch.zeros(4, 16, device=DEV)
    assert L.plb_launch_amax(x.data_ptr(), 0, 4, 12, 16, site.data_ptr(), stream()) != 0
    assert L.plb_launch_amax(x.data_ptr(), 0, 0, 8, 16, site.data_ptr(), stream()) != 0


# ---------------------------------------------------------------------------------------------------- quantize_multi
@pytest.mark.parametrize("case", ["one", "eight"])
def test_quantize_multi(case):
    L = _lib.lib()
    g = torch.Generator().manual_seed(6)
    if case == "one":
        specs = [(1 << 21) + 8 * 7, 0]                       # (elements, flags): one matrix, the 1024-block grid
        specs = [(specs[0], 1)]
    else:                                                    # bit 0: bf16 source, bit 1: e5m2 image
        specs = [(8, 1), (1000 * 8 + 8, 0), (128 * 256 * 8 + 24, 3), (56, 2), (768 * 768, 1), (4104, 0), (8, 2),
                 (2304 * 768 + 8, 3)]
    n = len(specs)
    srcs, scales, sref = [], [], []
    for i, (ne, fl) in enumerate(specs):
        x = torch.randn(ne, generator=g) * (10.0 ** (i % 3 - 1))
        x[int(torch.randint(ne, (1,), generator=g))] *= 8     # one element well above the rest
        x = x.to(torch.bfloat16) if fl & 1 else x
        srcs.append(x.to(DEV))
        sref.append(x)
        scales.append(float(np.float32(fp8_fmax(fl & 2) / (1.7 * float(x.float().abs().max())))))
    PAD = 64
    dsts = [torch.full((ne + PAD,), 0xC3, dtype=torch.uint8, device=DEV) for ne, _ in specs]
    sc = torch.tensor(scales, dtype=torch.float32, device=DEV)
    sites = torch.zeros(n + 1, SITE, device=DEV)               # one site more than matrices: must stay zero
    flags = (C.c_int * n)(*[fl for _, fl in specs])
    elems = (C.c_size_t * n)(*[ne for ne, _ in specs])
    rc = L.plb_launch_quantize_multi(n, ptr_array(srcs), flags, elems,
                                     (C.c_void_p * n)(*[sc.data_ptr() + 4 * i for i in range(n)]), ptr_array(dsts),
                                     (C.c_void_p * n)(*[sites[i].data_ptr() for i in range(n)]), stream())
    assert rc == 0
    torch.cuda.synchronize()
    for i, (ne, fl) in enumerate(specs):
        d = dsts[i].cpu()
        assert_fp8_image(d[:ne].reshape(1, ne), sref[i].reshape(1, ne), sc[i], fl & 2, slice(None), amax_site=sites[i])
        assert bool((d[ne:] == 0xC3).all()), i                 # bytes past the matrix untouched
    assert bool((sites[n] == 0).all())


def test_quantize_multi_refuses():
    L = _lib.lib()
    x = torch.zeros(16, device=DEV)
    d = torch.zeros(16, dtype=torch.uint8, device=DEV)
    s = torch.ones(1, device=DEV)
    site = torch.zeros(SITE, device=DEV)
    one = lambda t: (C.c_void_p * 1)(t.data_ptr())  # noqa: E731
    assert L.plb_launch_quantize_multi(1, one(x), (C.c_int * 1)(0), (C.c_size_t * 1)(12), one(s), one(d), one(site),
                                       stream()) != 0
    assert L.plb_launch_quantize_multi(0, one(x), (C.c_int * 1)(0), (C.c_size_t * 1)(16), one(s), one(d), one(site),
                                       stream()) != 0


# --------------------------------------------------------------------------------------- delayed scaling state machine
class ScalesModel:
    """plb_launch_fp8_scales2 restated from its contract (csrc/plbert_kernels.h, the comment above fp8_scales_kernel):
     * a group of `group` consecutive sites takes the maximum over all their slots; every slot is cleared, whatever it held;
     * groups whose first entry is at or past n2 use the second target fmax2 (and the format e5m2: 57344), the others
       fmax (e4m3: 448);
     * a maximum of 0 (nothing seen) or +inf leaves scale, deq and stats as they were;
     * stats, 8 words per group: [0..3] the history of maxima, slot (calls & 3); [4] calls with a * used / fmt > 1.0625,
       `used` the scale the call's values were quantised with (scale[first entry] before the update); [5] the worst such
       ratio; [6] the call counter as uint32;
     * groups at or past hist_from take their target from the largest of the four history entries, the others from a;
     * scale = fmax / target, deq = target / fmax, both in fp32 (correctly rounded: no fast-math in the build)."""

    def __init__(self, n, fmax, group, n2=None, fmax2=None, stats=False, hist_from=0):
        self.n, self.fmax, self.group = n, np.float32(fmax), group
        self.n2 = n if n2 is None else n2
        self.fmax2 = self.fmax if fmax2 is None else np.float32(fmax2)
        self.hist_from = hist_from
        self.ng = (n + group - 1) // group
        self.scale = np.zeros(n, np.float32)
        self.deq = np.zeros(n, np.float32)
        self.stats = np.zeros((self.ng, 8), np.float32) if stats else None

    def call(self, slots):
        """slots: [n, 64] float32 maxima held by the sites' slots before the call."""
        f32 = np.float32
        for gi in range(self.ng):
            g0, g1 = gi * self.group, min(gi * self.group + self.group, self.n)
            fm, fmt = (self.fmax2, f32(57344.0)) if g0 >= self.n2 else (self.fmax, f32(448.0))
            a = f32(max(0.0, float(slots[g0:g1].max())))
            if not (a > 0 and np.isfinite(a)):
                continue
            target = a
            if self.stats is not None:
                st = self.stats[gi]
                used = self.scale[g0]
                ratio = f32(f32(a * used) / fmt)
                if ratio > f32(1.0625):
                    st[4] = f32(st[4] + f32(1.0))
                    st[5] = max(st[5], ratio)
                calls = st[6:7].view(np.uint32)
                st[int(calls[0] & 3)] = a
                calls[0] += np.uint32(1)
                if gi >= self.hist_from:
                    target = f32(st[:4].max())
            self.scale[g0:g1] = f32(fm / target)
            self.deq[g0:g1] = f32(target / fm)


def _slots_for(maxima, g):
    """[n] -> [n, 64]: each site's maximum in one random slot, smaller values in a few others, zero elsewhere."""
    n = len(maxima)
    slots = np.zeros((n, F8_SLOTS), np.float32)
    for i, m in enumerate(maxima):
        if m == 0:
            continue
        k = g.choice(F8_SLOTS, size=4, replace=False)
        slots[i, k[0]] = m
        if np.isfinite(m):
            slots[i, k[1:]] = (np.float32(m) * g.uniform(0, 1, 3)).astype(np.float32)
    return slots


def _site_buffer(slots):
    n = slots.shape[0]
    buf = np.zeros((n, F8_SLOTS, F8_STRIDE), np.float32)
    buf[:, :, 0] = slots
    return torch.from_numpy(buf.reshape(n, SITE)).to(DEV)


def _one_ulp_above():
    f32 = np.float32
    # group 4 quantised at scale 28672 / 4 = 7168: find the smallest maximum above 8.5 whose ratio a * 7168 / 57344 rounds
    # above 1.0625 in fp32 (8.5 itself gives exactly 1.0625)
    a = f32(8.5)
    while f32(f32(a * f32(7168.0)) / f32(57344.0)) <= f32(1.0625):
        a = np.nextafter(a, f32(np.inf))
    return a


def _schedule(L, ncalls, g):
    """Engine layout (group L, n2 = 4 L): the maxima of the 8 groups per call, with the cases of the contract placed in
    known groups. Groups 0-3: e4m3 (target 448), 4-7: e5m2 (target 28672)."""
    f32 = np.float32
    above = _one_ulp_above()
    per_call = []
    for c in range(ncalls):
        gm = [f32(g.uniform(0.5, 2.0) * 10.0 ** g.integers(-3, 3)) for _ in range(8)]
        gm[1] = f32(0.0) if c < 3 or c in (6, 7) else gm[1]    # group 1: a group that sees nothing (incl. the first call)
        if c == 3:
            gm[2] = f32(np.inf)                                   # group 2: an infinite maximum
        gm[3] = f32(4.0) if c == 0 else (f32(4.25) if c == 1 else gm[3])   # ratio 4.25 * 112 / 448 = 1.0625 exactly
        gm[4] = f32(4.0) if c == 0 else (above if c == 1 else gm[4])       # one ulp above 1.0625
        gm[5] = f32(10.0) if c == 2 else f32(1.0)                           # rises, then falls: held four calls
        per_call.append(gm)
    return per_call


def _maxima_to_sites(gm, L, g):
    """group maxima -> per-site maxima (the group's maximum in one site of the group, smaller values in others)."""
    m = np.zeros(8 * L, np.float32)
    for gi, a in enumerate(gm):
        if a == 0:
            continue
        sites = np.arange(gi * L, gi * L + L)
        lead = g.choice(sites)
        m[lead] = a
        if np.isfinite(a):
            for s in sites:
                if s != lead and g.uniform() < 0.6:
                    m[s] = np.float32(a * g.uniform(0.0, 1.0))
    return m


def _launch_scales2(Lb, amax, scale, deq, n, fmax, group, n2, fmax2, stats, hist_from):
    rc = Lb.plb_launch_fp8_scales2(amax.data_ptr(), scale.data_ptr(), deq.data_ptr(), n, fmax, group, n2, fmax2,
                                   stats.data_ptr() if stats is not None else None, hist_from, stream())
    assert rc == 0
    torch.cuda.synchronize()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("L,hist_from", [(4, 0), (12, 0), (12, 5)])
def test_fp8_scales2_state_machine_in_the_engine_layout(L, hist_from):
    Lb = _lib.lib()
    g = np.random.default_rng(L * 10 + hist_from)
    n, ncalls = 8 * L, 12
    model = ScalesModel(n, 448.0, L, 4 * L, 28672.0, stats=True, hist_from=hist_from)
    scale = torch.zeros(n, device=DEV)
    deq = torch.zeros(n, device=DEV)
    stats = torch.zeros(8, 8, device=DEV)
    for c, gm in enumerate(_schedule(L, ncalls, g)):
        slots = _slots_for(_maxima_to_sites(gm, L, g), g)
        amax = _site_buffer(slots)
        _launch_scales2(Lb, amax, scale, deq, n, 448.0, L, 4 * L, 28672.0, stats, hist_from)
        model.call(slots)
        assert bool((amax == 0).all()), c                                  # every slot cleared
        assert _same_bits(scale.cpu().numpy(), model.scale), (c, scale.cpu().numpy(), model.scale)
        assert _same_bits(deq.cpu().numpy(), model.deq), c
        assert _same_bits(stats.cpu().numpy(), model.stats), (c, stats.cpu().numpy(), model.stats)
    # the cases the schedule was built to reach, checked on the model (the kernel equals it bit for bit above)
    st = model.stats
    calls = st[:, 6].copy().view(np.uint32)
    assert calls[1] == ncalls - 5 and calls[2] == ncalls - 1 and calls[0] == ncalls    # empty / infinite calls not counted
    assert st[0, 6].view(np.uint32) > 4                                                  # the counter wrapped past slot 3


def test_fp8_scales2_cases_one_by_one():
    """The individual rules, each visible in a short sequence at L = 4 (n = 32, group 4, n2 = 16, 448 / 28672)."""
    Lb = _lib.lib()
    L, n = 4, 32
    scale = torch.zeros(n, device=DEV)
    deq = torch.zeros(n, device=DEV)
    stats = torch.zeros(8, 8, device=DEV)
    model = ScalesModel(n, 448.0, L, 4 * L, 28672.0, stats=True, hist_from=0)
    g = np.random.default_rng(1)

    def run(gm):
        slots = _slots_for(_maxima_to_sites([np.float32(v) for v in gm], L, g), g)
        _launch_scales2(Lb, _site_buffer(slots), scale, deq, n, 448.0, L, 4 * L, 28672.0, stats, 0)
        model.call(slots)
        assert _same_bits(scale.cpu().numpy(), model.scale) and _same_bits(deq.cpu().numpy(), model.deq)
        assert _same_bits(stats.cpu().numpy(), model.stats)
        return scale.cpu().numpy().copy(), stats.cpu().numpy().copy()

    above = _one_ulp_above()
    s, st = run([4, 0, 4, 4, 4, 4, 4, 1])
    assert s[0] == 112.0 and s[4] == 0.0 and s[16] == 7168.0            # first call: from scale 0; group 1 saw nothing
    assert st[:, 4].sum() == 0                                           # nothing counted against scale 0
    s, st = run([4, 0, np.inf, 4.25, above, 4, 4, 1])
    assert s[8] == 112.0 and st[2, 6].view(np.uint32) == 1              # inf: scale and history unchanged
    assert st[3, 4] == 0 and st[4, 4] == 1 and st[4, 5] > 1.0625       # exactly 1.0625 not counted, one ulp above counted
    for c in range(6):
        s, st = run([4, 0, 4, 4, 4, 10 if c == 0 else 1, 4, 1])
        held = np.float32(28672.0) / np.float32(10.0)
        assert (s[20] == held) == (c < 4), (c, s[20])                   # a maximum is held for four calls, then released
    assert s[20] == np.float32(28672.0)


def test_fp8_scales_weight_update_group_one():
    """The weight images' update (csrc/engine_fp8.cpp: fp8_quantize_weights): group 1, no stats, target 448."""
    Lb = _lib.lib()
    n = 8
    g = np.random.default_rng(2)
    model = ScalesModel(n, 448.0, 1)
    scale = torch.zeros(n, device=DEV)
    deq = torch.zeros(n, device=DEV)
    for c in range(6):
        m = (g.uniform(0.01, 3.0, n)).astype(np.float32)
        m[c % n] = 0.0
        if c == 2:
            m[5] = np.inf
        slots = _slots_for(m, g)
        amax = _site_buffer(slots)
        assert Lb.plb_launch_fp8_scales(amax.data_ptr(), scale.data_ptr(), deq.data_ptr(), n, 448.0, 1, stream()) == 0
        torch.cuda.synchronize()
        model.call(slots)
        assert bool((amax == 0).all())
        assert _same_bits(scale.cpu().numpy(), model.scale), c
        assert _same_bits(deq.cpu().numpy(), model.deq), c


# ------------------------------------------------------------------------------ the image contract at the writers
# Each writer is asked for its bf16 output and its image in the same launch; the image buffer is filled with a sentinel,
# and only the rows the writer stores may change. The image must be ocp_bytes of the STORED bf16 values, and the site's
# maximum must equal max |stored| over those rows.
SENT = 0x6D


@pytest.mark.parametrize("H", [768, 1024])
@pytest.mark.parametrize("T", [1, 333, 4097])
def test_layernorm_forward_writes_the_fp8_image(H, T):
    L = _lib.lib()
    g = torch.Generator().manual_seed(H + T)
    x = (torch.randn(T, H, generator=g) * 2 + 0.5).to(torch.bfloat16).to(DEV)
    gam = (1 + 0.3 * torch.randn(H, generator=g)).to(DEV)
    bet = (0.2 * torch.randn(H, generator=g)).to(DEV)
    Tbuf = T + 5
    y = torch.full((Tbuf, H), 7.0, dtype=torch.bfloat16, device=DEV)
    img = torch.full((Tbuf, H), SENT, dtype=torch.uint8, device=DEV)
    mean = torch.zeros(Tbuf, device=DEV)
    rstd = torch.zeros(Tbuf, device=DEV)
    qs = torch.tensor([float(np.float32(448.0 / 3.1))], device=DEV)
    site = torch.zeros(SITE, device=DEV)
    p = _lib.PlbLayerNorm()
    p.x, p.ldx, p.gamma, p.beta, p.eps = x.data_ptr(), H, gam.data_ptr(), bet.data_ptr(), 1e-12
    p.y, p.ldy, p.mean, p.rstd, p.T, p.H, p.Tzero = y.data_ptr(), H, mean.data_ptr(), rstd.data_ptr(), T, H, T
    p.out8, p.ld8, p.q_scale, p.q_amax = img.data_ptr(), H, qs.data_ptr(), site.data_ptr()
    assert L.plb_launch_ln_fwd(C.byref(p), stream()) == 0
    torch.cuda.synchronize()
    assert_fp8_image(img, y, qs, 0, slice(0, T), amax_site=site, sentinel=SENT)


@pytest.mark.parametrize("H", [768, 1024])
@pytest.mark.parametrize("T,Tzero", [(333, 340), (4096, 4096 + 128), (5, 5)])
def test_layernorm_backward_writes_the_fp8_image(H, T, Tzero):
    """e5m2 image of dx; rows T..Tzero of the image are zero BYTES (the fp8 weight-gradient GEMMs sum over them)."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(H + T + 1)
    x = (torch.randn(T, H, generator=g) * 2).to(torch.bfloat16)
    xf = x.float()
    mean = xf.mean(1)
    rstd = (xf.var(1, unbiased=False) + 1e-12).rsqrt()
    dy = (torch.randn(T, H, generator=g) * 1e-3).to(torch.bfloat16)
    gam = 1 + 0.3 * torch.randn(H, generator=g)
    d = {k: v.to(DEV) for k, v in dict(x=x, mean=mean, rstd=rstd, dy=dy, gam=gam).items()}
    Tbuf = Tzero + 3
    dx = torch.full((Tbuf, H), 7.0, dtype=torch.bfloat16, device=DEV)
    img = torch.full((Tbuf, H), SENT, dtype=torch.uint8, device=DEV)
    nb = 64
    part = torch.zeros(nb, 3 * H, device=DEV)
    qs = torch.tensor([2.0 ** 20], device=DEV)
    site = torch.zeros(SITE, device=DEV)
    p = _lib.PlbLayerNorm()
    p.x, p.ldx, p.gamma, p.eps = d["x"].data_ptr(), H, d["gam"].data_ptr(), 1e-12
    p.mean, p.rstd, p.T, p.H, p.Tzero = d["mean"].data_ptr(), d["rstd"].data_ptr(), T, H, Tzero
    p.dy, p.lddy, p.dx, p.lddx, p.partials, p.nblocks = d["dy"].data_ptr(), H, dx.data_ptr(), H, part.data_ptr(), nb
    p.out8, p.ld8, p.q_scale, p.q_amax = img.data_ptr(), H, qs.data_ptr(), site.data_ptr()
    assert L.plb_launch_ln_bwd(C.byref(p), stream()) == 0
    torch.cuda.synchronize()
    im = img.cpu()
    assert bool((im[T:Tzero] == 0).all())
    im[T:Tzero] = SENT                                       # checked: the rest of the buffer must hold the sentinel
    assert_fp8_image(im, dx, qs, 1, slice(0, T), amax_site=site, sentinel=SENT)


def _qkv(B, S, NH, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B * S, 3 * NH * 64, generator=g)).to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("B,S,NH,lens", [(3, 130, 2, [130, 77, 1]), (2, 512, 12, [512, 300])])
def test_attention_forward_writes_the_fp8_image(B, S, NH, lens):
    """ctx8 = e4m3 image of the context rows (csrc/attn_common.h). The forward stores a context row for EVERY query row
    (lengths mask keys only): rows [0, B*S) are stored, the rows past them and the columns past H of the image stay."""
    from gpu_util import attn_args
    L = _lib.lib()
    H = NH * 64
    qkv = _qkv(B, S, NH, S + NH)
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    p, _, lse = attn_args(qkv, lengths, B, S, NH)
    ctx = torch.full((B * S + 3, H), 7.0, dtype=torch.bfloat16, device=DEV)
    ld8 = H + 16
    img = torch.full((B * S + 3, ld8), SENT, dtype=torch.uint8, device=DEV)
    qs = torch.tensor([float(np.float32(448.0 / 1.3))], device=DEV)
    site = torch.zeros(SITE, device=DEV)
    p.ctx, p.ldctx = ctx.data_ptr(), H
    p.ctx8, p.ldctx8, p.ctx_scale, p.ctx_amax = img.data_ptr(), ld8, qs.data_ptr(), site.data_ptr()
    assert L.plb_launch_attn_fwd(C.byref(p), stream()) == 0
    torch.cuda.synchronize()
    c = ctx.cpu()
    assert bool((c[B * S:] == 7.0).all()) and not bool((c[:B * S] == 7.0).all(1).any())
    assert_fp8_image(img, c, qs, 0, slice(0, B * S), amax_site=site, sentinel=SENT, cols=H)


@pytest.mark.parametrize("B,S,NH,lens,counts", [(3, 512, 2, [512, 300, 512], [70, 0, 140]),
                                                (4, 130, 3, [130, 77, 1, 129], [5, 33, 1, 0])])
def test_attention_backward_compact_queries_writes_the_fp8_images(B, S, NH, lens, counts):
    """Two-kernel backward in compact-query mode, rows and images in the same launch: dq8 = e5m2 image of the compact dq
    rows, dqkv8's K / V blocks the image of dqkv's K / V rows (padded keys: zero bytes); dqkv8's Q block is not written.
    Both images report into the one dqkv site: its maximum is the maximum over everything stored."""
    from gpu_util import attn_args
    L = _lib.lib()
    H = NH * 64
    qkv = _qkv(B, S, NH, 81 + S)
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(9)
    rows, off = [], [0]
    for b, n in enumerate(counts):
        pos = torch.randperm(lens[b], generator=g)[:n].sort().values
        rows += (pos + b * S).tolist()
        off.append(off[-1] + n)
    Nq = off[-1]
    rows_t = torch.tensor(rows, dtype=torch.int64, device=DEV)
    qoff = torch.tensor(off, dtype=torch.int32, device=DEV)
    qc = qkv[rows_t, :H].contiguous()
    pc, _, _ = attn_args(qkv, lengths, B, S, NH)
    ctxc = torch.zeros((Nq, H), dtype=torch.bfloat16, device=DEV)
    lsec = torch.zeros((NH, Nq), dtype=torch.float32, device=DEV)
    pc.ctx, pc.ldctx, pc.lse = ctxc.data_ptr(), H, lsec.data_ptr()
    pc.qoff, pc.q, pc.ldq, pc.nq_total = qoff.data_ptr(), qc.data_ptr(), H, Nq
    assert L.plb_launch_attn_fwd(C.byref(pc), stream()) == 0
    dctxc = (torch.randn(Nq, H, generator=g)).to(torch.bfloat16).to(DEV)
    delta = torch.zeros((NH, Nq), dtype=torch.float32, device=DEV)
    dq = torch.full((Nq + 2, H), 5.0, dtype=torch.bfloat16, device=DEV)
    dq8 = torch.full((Nq + 2, H), SENT, dtype=torch.uint8, device=DEV)
    dqkv = torch.full((B * S, 3 * H), 7.0, dtype=torch.bfloat16, device=DEV)
    dqkv8 = torch.full((B * S + 2, 3 * H), SENT, dtype=torch.uint8, device=DEV)
    scale = torch.tensor([2.0 ** 12], device=DEV)
    site = torch.zeros(SITE, device=DEV)
    pc.dctx, pc.lddctx, pc.delta, pc.dqkv, pc.lddqkv = dctxc.data_ptr(), H, delta.data_ptr(), dqkv.data_ptr(), 3 * H
    pc.dq, pc.lddq, pc.dq8, pc.lddq8 = dq.data_ptr(), H, dq8.data_ptr(), H
    pc.dqkv8, pc.lddqkv8, pc.dqkv_scale, pc.dqkv_amax = dqkv8.data_ptr(), 3 * H, scale.data_ptr(), site.data_ptr()
    assert L.plb_launch_attn_bwd(C.byref(pc), stream()) == 0
    torch.cuda.synchronize()
    d, dkv = dq.cpu(), dqkv.cpu()
    assert bool((d[Nq:] == 5.0).all()) and bool((dkv[:, :H] == 7.0).all())
    assert_fp8_image(dq8, d, scale, 1, slice(0, Nq), sentinel=SENT)
    assert_fp8_image(dqkv8[:, H:], dkv[:, H:], scale, 1, slice(0, B * S), sentinel=SENT)
    assert bool((dqkv8[:, :H] == SENT).all())                          # the Q block belongs to dq8 in this mode
    kpad = ~(torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).reshape(B * S)
    assert bool((dqkv8[:B * S].cpu()[kpad, H:] == 0).all())
    want_max = max(float(d[:Nq].float().abs().max()) if Nq else 0.0, float(dkv[:, H:].float().abs().max()))
    assert site_max(site) == want_max


@pytest.mark.parametrize("B,S,NH,lens", [(3, 130, 2, [130, 77, 1]), (4, 512, 4, [512, 512, 400, 77])])
def test_attention_backward_single_kernel_writes_the_fp8_image(B, S, NH, lens):
    """The single-kernel backward refuses rows and image together: run it with rows only, then with the image only. The
    image must be ocp_bytes of the first run's rows (the kernel is deterministic: test_attention_race_screen), padded rows
    zero bytes, rows past B*S untouched, and the site's maximum the maximum of those rows."""
    from gpu_util import attn_args
    L = _lib.lib()
    H = NH * 64
    qkv = _qkv(B, S, NH, 91 + S)
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    p, ctx, lse = attn_args(qkv, lengths, B, S, NH)
    assert L.plb_launch_attn_fwd(C.byref(p), stream()) == 0
    g = torch.Generator().manual_seed(92)
    qmask = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).reshape(B * S, 1)
    dctx = ((torch.randn(B * S, H, generator=g)) * qmask).to(torch.bfloat16).to(DEV)
    delta = torch.zeros((B, NH, S), dtype=torch.float32, device=DEV)
    dqkv = torch.full((B * S, 3 * H), 7.0, dtype=torch.bfloat16, device=DEV)
    p.dctx, p.lddctx, p.delta, p.dqkv, p.lddqkv = dctx.data_ptr(), H, delta.data_ptr(), dqkv.data_ptr(), 3 * H
    assert L.plb_launch_attn_bwd_fused(C.byref(p), stream()) == 0
    img = torch.full((B * S + 2, 3 * H), SENT, dtype=torch.uint8, device=DEV)
    scale = torch.tensor([float(np.float32(2.0 ** 12 / 1.7))], device=DEV)
    site = torch.zeros(SITE, device=DEV)
    p.dqkv = None
    p.dqkv8, p.lddqkv8, p.dqkv_scale, p.dqkv_amax = img.data_ptr(), 3 * H, scale.data_ptr(), site.data_ptr()
    assert L.plb_launch_attn_bwd_fused(C.byref(p), stream()) == 0
    torch.cuda.synchronize()
    rows = dqkv.cpu()
    assert not bool((rows == 7.0).all(1).any())                        # the rows-only run stored every row
    assert_fp8_image(img, rows, scale, 1, slice(0, B * S), amax_site=site, sentinel=SENT)
    kpad = ~qmask.reshape(B * S)
    assert bool((img[:B * S].cpu()[kpad] == 0).all())                 # padded keys (and queries): zero bytes
