"""tests/stride_ref.py without a GPU: planes and blocks lie where the layout says, everything else is poison, and
the guard check catches a planted write (and only a planted write)."""
import numpy as np
import pytest

import stride_ref as sr


@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.uint8])
@pytest.mark.parametrize("form", sr.FORMS)
def test_embed_stack_places_planes(dtype, form):
    C, N, P = 2, 5, 36
    pads = sr.form_pads(form, 16 if dtype == np.uint8 else 4)
    dense = np.random.default_rng(1).integers(0, 101, (C, N, P)).astype(dtype)
    buf, b, ls, cs = sr.embed_stack(dense, pads["lpad"], pads["cpad"], pads["off"])
    assert ls == P + pads["lpad"] and cs == N * ls + pads["cpad"] and buf.dtype == dense.dtype
    for c in range(C):
        for n in range(N):
            at = pads["off"] + c * cs + n * ls
            assert np.array_equal(buf[at:at + P], dense[c, n])
    assert np.array_equal(b.gather(buf), dense)
    rest = buf[~b.payload_mask()]
    assert rest.size == buf.size - C * N * P and rest.size >= sr.GUARD
    if dtype == np.float32:
        assert np.isnan(rest).all()
    else:
        assert (rest == sr.POISON[np.dtype(dtype)]).all()
    inside, b2, _, _ = sr.embed_stack(dense, 1, 0, 0, poison=28)  # a poison the caller picks (inside a window)
    assert (inside[~b2.payload_mask()] == 28).all() and inside[P] == 28 and np.array_equal(b2.gather(inside), dense)


def test_form_pads_keep_or_break_the_vector_predicates():
    for vec in (4, 16):
        a = sr.form_pads("aligned", vec)
        assert all(a[n] % vec == 0 for n in ("lpad", "cpad", "off")) and a["opad"] % 4 == 0 and a["ooff"] % 4 == 0
        assert a["lpad"] > 0 and a["cpad"] > 0 and a["opad"] > 0
    assert sr.form_pads("oddlight")["lpad"] % 2 == 1
    f = sr.form_pads("offset")
    assert f["off"] % 4 and f["ooff"] % 4 and (f["cpad"] % 4 or f["opad"] % 4)


def test_out_blocks_and_guards():
    C, block = 2, 30
    b, ocs = sr.out_blocks(C, block, pad=2, off=1)
    assert ocs == 32 and b.start == sr.GUARD + 1 and b.size == sr.GUARD + 1 + ocs + block + sr.GUARD
    buf = sr.nan_buffer(b)
    assert buf.dtype == np.float32 and np.isnan(buf).all() and sr.untouched(buf)
    assert sr.clobbered(buf, b).size == 0
    buf[b.index()] = np.arange(C * block, dtype=np.float32).reshape(C, block)
    assert sr.clobbered(buf, b).size == 0 and not sr.untouched(buf)  # payload writes are not guard writes
    assert np.array_equal(b.gather(buf)[1], np.arange(block, 2 * block))
    for at in (0, b.start - 1, b.start + block, b.start + ocs - 1, b.start + ocs + block, b.size - 1):
        planted = buf.copy()
        planted[at] = 0.0
        assert sr.clobbered(planted, b).tolist() == [at]
    # a NaN with another bit pattern in a gap is a write too (the comparison is on the int32 view)
    planted = buf.copy()
    planted.view(np.int32)[b.start + block] = 0x7FC00001
    assert sr.clobbered(planted, b).tolist() == [b.start + block]
    kept = sr.nan_buffer(b, np.int32)
    kept[3] = 7
    assert sr.clobbered(kept, b).tolist() == [3]


def test_out_rows_gaps_between_rows_and_channels():
    C, E, P = 2, 3, 8
    b, orow, ocs = sr.out_rows(C, E, P, rpad=1, cpad=5, off=0)
    assert orow == 9 and ocs == 32 and b.index().shape == (C, E, P)
    assert b.index()[1, 2, 0] == sr.GUARD + ocs + 2 * orow
    buf = sr.nan_buffer(b)
    buf[b.index()] = 1.0
    assert sr.clobbered(buf, b).size == 0
    buf[sr.GUARD + P] = 1.0  # the gap after row 0
    buf[sr.GUARD + E * orow] = 1.0  # the gap between the channels
    assert sr.clobbered(buf, b).tolist() == [sr.GUARD + P, sr.GUARD + E * orow]


def test_overlapping_or_outside_layouts_are_refused():
    with pytest.raises(AssertionError):
        sr.Blocks((2,), (10,), 11, 0, 64)
    with pytest.raises(AssertionError):
        sr.Blocks((2,), (10,), 10, 0, 19)
