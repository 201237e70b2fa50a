"""tests/far_ref.py without a GPU: every plan tests/test_gpu_far_strides.py uses passes both limits, absorbs every
32-bit truncation of its offsets inside its own poison, keeps or breaks the 16-byte predicates of rti_stack.h as
its variant says, and fits under the memory cap.  Run with -s to see each plan's offsets and truncations."""
import pytest

import far_ref as fr


def test_truncations_known_values():
    assert fr.truncations(5, 4) == (5, 5, 5, 5)
    assert fr.truncations((1 << 31) + 8, 4) == ((1 << 31) + 8, -(1 << 31) + 8, 8, 8)
    assert fr.truncations((1 << 30) + 4, 4) == ((1 << 30) + 4, (1 << 30) + 4, 4, 4)
    assert fr.truncations((1 << 32) + 3, 1) == (3, 3, 3, 3)
    assert fr.truncations((1 << 31) + 3, 1) == ((1 << 31) + 3, -(1 << 31) + 3, (1 << 31) + 3, -(1 << 31) + 3)
    assert fr.truncations((1 << 29) + 2, 8) == ((1 << 29) + 2, (1 << 29) + 2, 2, 2)


def test_stride_choices():
    """the figures the module's docstring states"""
    assert fr.far_channel_stride(4, 2, 100) == (1 << 31) + 100 + 4
    assert fr.far_channel_stride(4, 3, 100) == (1 << 30) + 100 + 4
    assert fr.far_channel_stride(1, 2, 100) == (1 << 32) + 112 + 16
    assert fr.far_channel_stride(8, 2, 100) == (1 << 29) + 100 + 4
    assert fr.far_channel_stride(4, 2, 100, "odd") == (1 << 31) + 100 + 5
    for es, n in ((4, 20), (4, 37), (1, 20), (1, 6), (4, 3)):
        L = fr.far_row_stride(es, n, 1316)
        assert (n - 1) * L > fr.LIM_ELEMS and (n - 1) * L * es > fr.LIM_BYTES
        vec = 16 // es
        assert (n - 1) * (L - fr._up(1316, vec) - 2 * vec) < max(fr.LIM_ELEMS, fr.LIM_BYTES // es), "not the smallest"


@pytest.mark.parametrize("name", sorted(fr.PLANS))
def test_plan(name):
    p = fr.PLANS[name]
    print("\n" + p.describe())
    first = [int(e) for e in p.block_offsets().ravel()]
    # both limits are passed by some block (8-byte elements: the byte limit only, see far_ref)
    assert max(first) * p.es > fr.LIM_BYTES, "no block past 2^32 bytes"
    if p.es <= 4:
        assert max(first) > fr.LIM_ELEMS, "no block past 2^31 elements"
    # blocks do not overlap and lie inside the allocation, the guard before and after included
    srt = sorted(first)
    assert all(b - a >= p.inner for a, b in zip(srt, srt[1:])), "blocks overlap"
    assert p.base >= 64 and p.base + srt[-1] + p.inner + 64 <= p.length
    assert (p.base * p.es) % 16 == 0, "the payload base is 16-byte aligned; only the strides make a variant odd"
    # every truncation of every block's first and last element is inside the allocation and in poison
    wrong = 0
    for e in p.corner_offsets():
        for t in fr.truncations(e, p.es):
            assert 0 <= p.base + t < p.length, (name, e, t, "outside the allocation")
            if t != e:
                wrong += 1
                assert not p.in_payload(t), (name, e, t, "a truncated offset lands in a payload")
    assert wrong > 0, "no truncation differs from the true offset: the plan cannot show a defect"
    # the far stride keeps (aligned) or breaks (odd) the 16-byte predicates of rti_stack.h
    vec = 16 // p.es if p.es <= 4 else 4
    far = p.strides[p.far]
    assert far * (p.counts[p.far] - 1) * p.es > fr.LIM_BYTES, "the far stride does not reach the limits"
    if name.endswith("-aligned"):
        assert all(s % vec == 0 for s in p.strides if s != p.inner or p.inner % vec == 0), p.strides
    else:
        assert name.endswith("-odd") and far % vec == 1, p.strides
    assert p.nbytes() <= fr.CAP_BYTES, f"{p.nbytes() / 2**30:.1f} GiB"
