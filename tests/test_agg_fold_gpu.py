"""``hs_agg_fold`` (csrc/kernels/scan_filter.hip) against ``hs_agg_final`` and the numpy model of
their common order (``tests/test_agg_fold.py``), bit for bit."""
import ctypes as C

import numpy as np
import pytest

from hyperspace_amd.ops import _lib as NL
from test_agg_fold import fold_model, make_partials

NBLK = (1, 63, 64, 255, 256, 257, 1000)
GAS = (1, 3, 5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("sum", "count", "min", "max")):
        assert np.array_equal(_bits(g), _bits(w)), (what, name, g, w)


def _split(buf: np.ndarray, GA: int):
    n = 8 * GA
    return (buf[0:n].view(np.float64), buf[n:2 * n].view(np.int64),
            buf[2 * n:3 * n].view(np.float64), buf[3 * n:4 * n].view(np.float64))


@pytest.fixture(scope="module")
def reference():
    """Per shape and set: the partials on the device, ``hs_agg_final``'s result and the model's,
    computed once."""
    from conftest import gpu_available
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from hyperspace_amd.ops import kernels as K
    device = torch.device("cuda:0")
    L = NL.lib()
    ref = {}
    for nblk in NBLK:
        for GA in GAS:
            for k in (0, 1):
                host = make_partials(nblk, GA, 1000 * nblk + 10 * GA + k)
                dev = tuple(torch.from_numpy(x).to(device) for x in host)
                out = K.agg_outputs(GA, device)
                NL.check(L.hs_agg_final(*(NL.ptr(x) for x in dev), nblk, GA,
                                        *(NL.ptr(x) for x in out), NL.stream_ptr()), "hs_agg_final")
                torch.cuda.synchronize()
                final = _split(out[0].hs_buf.cpu().numpy(), GA)
                ref[nblk, GA, k] = (dev, final, fold_model(*host, nblk, GA))
    return ref


def _set(dev, nblk, dout, hout):
    return NL.AggFoldSet(*(x.data_ptr() for x in dev), dout, hout, nblk, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("nsets", [1, 2])
def test_fold_equals_final_and_the_model_bit_for_bit(device, reference, nsets):
    import torch
    from hyperspace_amd.exec.graphs import _Pinned
    L = NL.lib()
    some_inf, some_negzero, some_big = False, False, False
    for nblk in NBLK:
        for GA in GAS:
            nbytes = 32 * GA
            douts = [torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=device)
                     for _ in range(nsets)]
            houts = [_Pinned(nbytes) for _ in range(nsets)]
            for h in houts:
                h.view()[:] = 0xA5
            a = NL.AggFoldArgs(GA, nsets)
            for k in range(nsets):
                a.set[k] = _set(reference[nblk, GA, k][0], nblk, douts[k].data_ptr(), houts[k].ptr)
            NL.check(L.hs_agg_fold(C.byref(a), NL.stream_ptr()), "hs_agg_fold")
            torch.cuda.synchronize()
            for k in range(nsets):
                _, final, model = reference[nblk, GA, k]
                host = _split(houts[k].view().copy(), GA)
                _same(host, final, (nblk, GA, k, "host block vs hs_agg_final"))
                _same(_split(douts[k].cpu().numpy(), GA), final,
                      (nblk, GA, k, "device block vs hs_agg_final"))
                _same(host, model, (nblk, GA, k, "host block vs model"))
                some_inf |= bool(np.isinf(host[2]).any() or np.isinf(host[3]).any())
                some_negzero |= bool((_bits(host[2]) == 1 << 63).any() or
                                     (_bits(host[3]) == 1 << 63).any())
                some_big |= bool((host[1] > (1 << 40)).any())
    # the inputs reach the results' edge cases: a slot no block saw, -0.0 as an extreme, counts
    # above 2^40
    assert some_big and (some_inf or some_negzero)


@pytest.mark.gpu
def test_second_set_with_a_null_device_block_writes_only_its_host_block(device, reference):
    import torch
    from hyperspace_amd.exec.graphs import _Pinned
    L = NL.lib()
    for nblk, GA in ((257, 3), (1, 1), (1000, 5)):
        nbytes = 32 * GA
        dout = torch.full((2 * nbytes,), 0xA5, dtype=torch.uint8, device=device)
        ha, hb = _Pinned(nbytes), _Pinned(nbytes)
        ha.view()[:] = 0xA5
        hb.view()[:] = 0xA5
        a = NL.AggFoldArgs(GA, 2)
        a.set[0] = _set(reference[nblk, GA, 0][0], nblk, dout.data_ptr(), ha.ptr)
        a.set[1] = _set(reference[nblk, GA, 1][0], nblk, None, hb.ptr)
        NL.check(L.hs_agg_fold(C.byref(a), NL.stream_ptr()), "hs_agg_fold")
        torch.cuda.synchronize()
        d = dout.cpu().numpy()
        _same(_split(d[:nbytes], GA), reference[nblk, GA, 0][1], "set 0 device block")
        assert (d[nbytes:] == 0xA5).all()       # nothing of set 1 reached device memory beside it
        _same(_split(ha.view().copy(), GA), reference[nblk, GA, 0][1], "set 0 host block")
        _same(_split(hb.view().copy(), GA), reference[nblk, GA, 1][1], "set 1 host block")


@pytest.mark.gpu
def test_launcher_rejects_malformed_blocks(device):
    L = NL.lib()
    a = NL.AggFoldArgs(1, 3)
    assert L.hs_agg_fold(C.byref(a), NL.stream_ptr()) != 0
    a = NL.AggFoldArgs(1, 1)          # no host block
    assert L.hs_agg_fold(C.byref(a), NL.stream_ptr()) != 0
