"""tests/lowp_util.quantize (numpy only) against torch.Tensor.to(dtype), no GPU: 10^6 seeded values in [0, 1],
the ties of the rounding, the subnormals of both formats."""
import numpy as np
import pytest

import lowp_util


def _torch_bits(a, dtype):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(lowp_util.torch_dtype(dtype))
    return t.view(torch.int16).numpy().view(np.uint16), t.float().numpy()


def _cases(dtype):
    rng = np.random.RandomState(20240607)
    vals = [rng.random_sample(1000000).astype(np.float32),
            (rng.random_sample(20000) * 1e-4).astype(np.float32),          # float16 subnormals lie below 6.1e-5
            np.float32(2.0) ** rng.randint(-140, 1, 20000).astype(np.float32)]
    # every midpoint between two neighbouring 16-bit values of [0, 1] (the ties), and its float32 neighbours
    pat = lowp_util.unit_interval_patterns(dtype)
    w = lowp_util.widen(pat, dtype).astype(np.float64)
    mid = ((w[:-1] + w[1:]) * 0.5).astype(np.float32)
    vals += [mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(1)), w.astype(np.float32)]
    # float32 subnormals (bfloat16 has them too) and the ends
    vals.append(np.array([0.0, 1e-45, 1e-40, 1.1754944e-38, 5.9604645e-08, 2.9802322e-08, 1.0, 1.0 - 2.0 ** -24,
                          1.0 - 2.0 ** -9, 1.0 - 2.0 ** -12], np.float32))
    return np.concatenate(vals)


@pytest.mark.parametrize("dtype", lowp_util.DTYPES)
def test_quantize_equals_torch(dtype):
    a = _cases(dtype)
    bits, wide = lowp_util.quantize(a, dtype)
    tbits, twide = _torch_bits(a, dtype)
    assert np.array_equal(bits, tbits)
    assert np.array_equal(wide.view(np.uint32), twide.view(np.uint32))
    assert np.array_equal(lowp_util.widen(bits, dtype).view(np.uint32), wide.view(np.uint32))


@pytest.mark.parametrize("dtype,count", [("float16", 15361), ("bfloat16", 16257)])
def test_unit_interval_patterns(dtype, count):
    pat = lowp_util.unit_interval_patterns(dtype)
    w = lowp_util.widen(pat, dtype)
    assert pat.size == count and w[0] == 0.0 and w[-1] == 1.0 and np.all(np.diff(w) > 0)
    bits, wide = lowp_util.quantize(w, dtype)            # a 16-bit value quantises to itself
    assert np.array_equal(bits, pat) and np.array_equal(wide, w)


@pytest.mark.parametrize("name", lowp_util.names())
def test_vectors_quantise_as_torch_does(name):
    v = lowp_util.load(name)                             # (asserts the sha256 of the 16-bit input bytes)
    cp, sp, _ = lowp_util.float_inputs(v["spec"])
    assert np.array_equal(_torch_bits(cp, v["dtype"])[0], v["class_bits"])
    assert np.array_equal(_torch_bits(sp, v["dtype"])[0], v["same_bits"])
