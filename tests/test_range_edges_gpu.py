"""Range tracking at its edges: dgp_tensor_absmax and the fp32 <-> H1 / H2 converters (dgp_ops.hip, dgp_device.h).

The fp16 tiers stay correct only because a tensor that leaves its cells is noticed.  Pinned here, bit for bit:
  * absmax: the scalar tail (n % 4 != 0, done by one thread), the grid-stride loop behind the 2048-block cap, the bit-pattern
    atomicMax over the slots (-0.0, denormals, inf);
  * the converters' rounding: H1 cell = fp16(x * 2^e) round-to-nearest-even; H2 high cell = the same, low cell = fp16(x * 2^e - high)
    (oracle/emul_split.py's split_f16, cell by cell) -- on every fp16 value and tie, -0.0 included (which an fma addend of +0
    once turned into +0);
  * the range edge: 65504 is the last finite cell, everything from the rounding boundary 65520 on is inf -- the event that
    h2_range_check_kernel's `< 60000` test on the tracked maximum guards -- and values below half the smallest fp16 subnormal
    become a zero that keeps its sign.
References are torch's CPU conversions (IEEE round-to-nearest-even) and float64."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE_EXPS = (0, 5, -7)


@pytest.fixture(scope="module")
def eng(lib_built):
    from deepgraphpose_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine


def _absmax(eng, x):
    """dgp_tensor_absmax on a device tensor (zeroed slots; the answer is the maximum over the slots) -> its fp32 bit pattern"""
    from deepgraphpose_amd import _lib
    slots = torch.zeros(eng.ABSMAX_SLOTS, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().dgp_tensor_absmax(x.data_ptr(), x.numel(), slots.data_ptr(), torch.cuda.current_stream().cuda_stream), "dgp_tensor_absmax")
    s = slots.cpu()
    assert not torch.isnan(s).any()
    return int(s.view(torch.int32).max())       # non-negative floats order like their bit patterns


def _bits_of(v):
    return int(np.array(v, dtype=np.float32).view(np.int32))


BIG = 2048 * 256 * 4 + 1203         # more float4s than 2048 blocks x 256 threads hold at once (grid-stride), and a 3-element tail


@pytest.fixture(scope="module")
def absmax_base():
    """N(0, 1) values, |x| < 6, shared by the cases (each one plants its extreme and takes it out again)"""
    x = torch.randn(BIG, generator=torch.Generator().manual_seed(31)).clamp_(-6.0, 6.0)
    return x, x.cuda()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, BIG])
def test_absmax_extreme_at_first_last_and_middle_element(eng, absmax_base, n):
    host, dev = absmax_base
    x = dev[:n]
    for pos in sorted({0, n // 2, n - 1}):
        keep = float(host[pos])
        x[pos] = -37.625
        ref = host[:n].clone()
        ref[pos] = -37.625
        want = ref.double().abs().max()
        try:
            got = _absmax(eng, x)
        finally:
            x[pos] = keep
        assert float(want) == 37.625 and got == _bits_of(float(want)), (n, pos, hex(got))
    # and without a planted extreme: the maximum of the random values, wherever it lies
    assert _absmax(eng, x) == _bits_of(float(host[:n].double().abs().max())), n


@pytest.mark.parametrize("n", [5, 1023])
@pytest.mark.parametrize("pos", ["first", "last"])
def test_absmax_zero_denormal_and_inf(eng, n, pos):
    """`last` lies in the scalar tail (n % 4 != 0), `first` in the float4 loop"""
    i = 0 if pos == "first" else n - 1
    x = torch.zeros(n, dtype=torch.float32)
    x[i] = -0.0
    x[n // 2] = -0.0
    assert _absmax(eng, x.cuda()) == 0                                  # all zeros, -0.0 among them: +0.0, bit pattern 0
    tiny = float(np.array(0x00000123, dtype=np.int32).view(np.float32))  # a denormal
    x[i] = -tiny
    x[n // 2] = tiny / 2
    assert float(x.double().abs().max()) == tiny
    assert _absmax(eng, x.cuda()) == 0x00000123
    x[n // 2] = 3.0e38
    x[i] = -float("inf")
    assert float(x.double().abs().max()) == float("inf")
    assert _absmax(eng, x.cuda()) == 0x7F800000


# ---------------------------------------------------------------------------- converters
def _fp16_values_and_midpoints():
    """Every finite fp16 value (both signs, subnormals and both zeros) widened to fp32, and every midpoint between neighbouring
    finite fp16 values (exact in fp32: 12 significant bits) -- the ties of round-to-nearest-even; padded with zeros to a multiple of 8."""
    pos = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)
    mid = (pos[:-1].astype(np.float64) + pos[1:].astype(np.float64)) / 2
    assert np.array_equal(mid.astype(np.float32).astype(np.float64), mid)
    v = np.concatenate([pos, -pos, mid.astype(np.float32), -mid.astype(np.float32)])
    return np.concatenate([v, np.zeros(-len(v) % 8, dtype=np.float32)])


def _ints22():
    """22-bit integers scaled into [2^10, 2^11), both signs: what an H2 cell pair holds exactly"""
    k = torch.randint(2 ** 21, 2 ** 22, (4096,), generator=torch.Generator().manual_seed(37)).double()
    k[:4] = torch.tensor([2.0 ** 21, 2.0 ** 22 - 1, 2.0 ** 21 + 1, 2.0 ** 22 - 2 ** 10 - 1])
    sign = torch.where(torch.arange(4096) % 3 == 0, -1.0, 1.0).double()
    return (k * sign * 2.0 ** -11).float().numpy()


def _prescaled(v, e):
    """x with x * 2^e == v exactly (a power of two moves only the exponent; none of these leaves the normal fp32 range)"""
    x = (v.astype(np.float64) * 2.0 ** -e).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 2.0 ** e, v.astype(np.float64))
    return torch.from_numpy(x)


def _h2_cells(eng, x, e):
    """dgp_f32_to_h2 -> (high, low) cells as int16 bit patterns in x's order (a cell pair: 8 high halves, then 8 low halves)"""
    raw = eng.f32_to_h2(x.cuda(), e).view(torch.int16).cpu().reshape(-1, 2, 8)
    return raw[:, 0].reshape(-1), raw[:, 1].reshape(-1)


def _h2_emul(x, e):
    """split_f16 of oracle/emul_split.py, the cells themselves: x * 2^e is exact, high = fp16(x s), low = fp16(x s - high)"""
    xs = x.double() * 2.0 ** e
    assert torch.equal(xs.float().double(), xs)
    hi = xs.float().half()
    r = xs - hi.double()
    fin = torch.isfinite(r)
    assert torch.equal(r[fin].float().double(), r[fin])          # the remainder is exact in fp32, as in the kernel's fma
    return hi.view(torch.int16), r.float().half().view(torch.int16)


def _same_bits(got, want, v):
    """int16 cell patterns equal; on failure: how many differ and the first few (input, got, want)"""
    bad = (got != want).nonzero().reshape(-1)[:6].tolist()
    assert not bad, (int((got != want).sum()), [(float(v[i]), hex(int(got[i]) & 0xFFFF), hex(int(want[i]) & 0xFFFF)) for i in bad])


@pytest.mark.parametrize("e", SCALE_EXPS)
def test_h1_converter_rounds_to_nearest_even_bit_for_bit(eng, e):
    v = _fp16_values_and_midpoints()
    x = _prescaled(v, e)
    want = (x * 2.0 ** e).half()
    assert torch.isfinite(want).all()
    got = eng.f32_to_h1(x.cuda(), e).cpu()
    _same_bits(got.view(torch.int16), want.view(torch.int16), v)
    # h1_to_f32 is the exact inverse on every fp16 value
    h = torch.from_numpy(np.concatenate([np.arange(0, 0x7C00, dtype=np.uint16), np.arange(0x8000, 0xFC00, dtype=np.uint16)]).view(np.float16))
    back = eng.h1_to_f32(h.cuda(), e).cpu()
    ref = (h.double() * 2.0 ** -e).float()
    assert torch.equal(ref.double(), h.double() * 2.0 ** -e)
    assert torch.equal(back.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(eng.f32_to_h1(back.cuda(), e).cpu().view(torch.int16), h.view(torch.int16))


@pytest.mark.parametrize("e", SCALE_EXPS)
def test_h2_converter_cells_bit_for_bit(eng, e):
    for v in (_fp16_values_and_midpoints(), _ints22()):
        x = _prescaled(v, e)
        hi, lo = _h2_cells(eng, x, e)
        hi_ref, lo_ref = _h2_emul(x, e)
        _same_bits(hi, hi_ref, v)
        _same_bits(lo, lo_ref, v)
        # the H1 cell IS the high cell
        assert torch.equal(eng.f32_to_h1(x.cuda(), e).cpu().view(torch.int16), hi)
        # h2_to_f32 returns (high + low) * 2^-e, exact in fp32
        back = eng.h2_to_f32(eng.f32_to_h2(x.cuda(), e), e).cpu()
        cells = hi_ref.view(torch.float16).double() + lo_ref.view(torch.float16).double()
        assert torch.equal(back.view(torch.int32), (cells * 2.0 ** -e).float().view(torch.int32))
        # <= 22 significant bits: the round trip is exact -- the 22-bit integers of the format's top binade, and every fp16 value or
        # midpoint from 2^-13 up (below, half an ulp of the high cell is no fp16 value any more: the low cell underflows)
        exact = torch.from_numpy(np.abs(v) >= 2.0 ** -13) | (x == 0)
        assert bool(exact.sum() > 0.85 * len(v))
        assert torch.equal(back[exact], x[exact])


@pytest.mark.parametrize("e", SCALE_EXPS)
def test_cells_at_the_fp16_range_edge(eng, e):
    """The cells' contract at both ends of the fp16 range, for x * 2^e =
         65504                      the largest finite cell
         just below 65520           still 65504
         65520 and just above       the rounding boundary: inf (high cell of H2, and the H1 cell)
         2^-24, 1.5 * 2^-25         the smallest subnormal; the first value that rounds up to it
         2^-25 and below            0 (2^-25 is a tie: to even), the sign kept"""
    f32 = np.float32
    up, down = np.nextafter(f32(65520), f32(np.inf)), np.nextafter(f32(65520), f32(0))
    v = np.array([65504, down, 65520, up, 2.0 ** 16, 3e9,
                  2.0 ** -24, 1.5 * 2.0 ** -25, 2.0 ** -25, np.nextafter(f32(2.0 ** -25), f32(0)), 2.0 ** -26, 1e-30], dtype=np.float32)
    want = np.array([65504, 65504, np.inf, np.inf, np.inf, np.inf, 2.0 ** -24, 2.0 ** -24, 0, 0, 0, 0], dtype=np.float16)
    v, want = np.concatenate([v, -v]), np.concatenate([want, -want])
    x = _prescaled(v, e)
    assert np.array_equal((x * 2.0 ** e).half().numpy().view(np.int16), want.view(np.int16))       # torch's CPU rounding agrees with the table
    h1 = eng.f32_to_h1(x.cuda(), e).cpu().numpy()
    hi, lo = _h2_cells(eng, x, e)
    assert np.array_equal(h1.view(np.int16), want.view(np.int16))
    assert np.array_equal(hi.numpy(), want.view(np.int16))
    hi_ref, lo_ref = _h2_emul(x, e)
    assert torch.equal(hi, hi_ref) and torch.equal(lo, lo_ref)
    # an overflowed pair is inf - inf: the value is gone, which is why the range check must fire first
    back = eng.h2_to_f32(eng.f32_to_h2(x.cuda(), e), e).cpu().numpy()
    assert np.array_equal(np.isnan(back), np.isinf(want.astype(np.float32)))
    # below the cells' resolution: a signed zero in both cells and after the round trip
    small = np.abs(v) <= 2.0 ** -25
    assert not (lo.numpy()[small] & 0x7FFF).any()
    assert np.array_equal(np.signbit(back[small]), np.signbit(v[small])) and not back[small].any()
