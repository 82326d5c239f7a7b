"""Host-side helpers of the kernel wrappers (ops/kernels.py) that need no GPU."""
def test_gather_probe_sample_positions_stay_in_range():
    """The packed-gather probe's sample positions (ops/kernels.py sample_positions) stay in
    [0, n - 2] for table sizes where a float32 linspace would round past the end."""
    import torch
    from hyperspace_amd.ops import kernels as K
    for n in (2, 3, 5, 4097, 16_777_217, 60_000_000, 600_037_902):
        pos = K.sample_positions(n, K.PACKED_SAMPLE, "cpu")
        assert int(pos.min()) >= 0 and int(pos.max()) <= n - 2, n
        assert pos.numel() == min(K.PACKED_SAMPLE, n - 1)
    assert K._random_permutation(torch.randperm(1 << 20))
    assert not K._random_permutation(torch.arange(1 << 20, dtype=torch.int32))


def test_float_key_image_range_is_the_ieee_predicate():
    """Range pruning on a float sort key (ops/kernels.py float_key_image_range): the keys whose
    image lies in the returned range are exactly the keys the IEEE comparison accepts - both
    zeros for a zero literal, no NaN of either sign - on the special-value ladder of the
    independent reference; a NaN literal gives no range."""
    import operator

    import numpy as np
    from hyperspace_amd.ops import _lib as NL, kernels as K
    from order_ref import SPECIAL_F32, SPECIAL_F64, ref_image
    ops = {NL.OP_EQ: operator.eq, NL.OP_LT: operator.lt, NL.OP_LE: operator.le,
           NL.OP_GT: operator.gt, NL.OP_GE: operator.ge}
    for kind, special in (("F64", SPECIAL_F64), ("F32", SPECIAL_F32)):
        hs = getattr(NL, kind)
        keys = np.concatenate([special, np.array([-2.5, -1.0, 1.0, 2.5], special.dtype)])
        img = [int(i) for i in ref_image(keys, kind)]
        for lit in keys:
            for op, fn in ops.items():
                rng = K.float_key_image_range(op, float(lit), hs)
                if np.isnan(lit):
                    assert rng is None
                    continue
                lo, hi = rng
                assert 0 <= lo < 2**64 and 0 <= hi < 2**64
                with np.errstate(invalid="ignore"):
                    want = fn(keys, lit)
                got = np.array([lo <= i <= hi for i in img])
                assert np.array_equal(got, want), (kind, float(lit), op, keys[got != want])
    # a literal that is no float32 cannot become an image of an F32 key
    for lit in (0.1, 1e300, -1e300, 1e-60):
        assert K.float_key_image_range(NL.OP_GT, lit, NL.F32) is None
    assert K.float_key_image_range(NL.OP_GT, 0.5, NL.F32) is not None
    assert K.float_key_image_range(NL.OP_GT, float("inf"), NL.F32) is not None
