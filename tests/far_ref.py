"""Far strides for the stack entries of include/rti.h: plans, without any allocation, of tiny payloads placed so
that the element offsets the kernels must form pass 2^31 elements and 2^32 bytes.

A `Plan` is the far sibling of stride_ref.Blocks: payload element (i0, i1, .., j), i_d < counts[d] and j < inner,
sits at element `base` + Σ_d i_d·strides[d] + j of an allocation of `length` elements of `es` bytes; the entry is
given the address of element `base` and the strides.  Everything else is poison (inputs) or NaN guard (outputs).

The allocation absorbs truncation.  For the first and the last element of every block, with true element offset e
from the entry's pointer, a kernel that keeps only 32 bits of e or of the byte offset e·es, read back as unsigned
or as signed, lands at one of

    u32(e)    s32(e)    u32(e·es) / es    s32(e·es) / es          (`truncations`)

elements from the pointer.  `base` is at least 2^31 elements or 2^31 bytes into the allocation wherever a signed
truncation is negative, and `length` covers the largest of them, so each of these lies in [0, length); the pad of
each far stride is longer than the payload it steps over, so a truncation that is not the true offset lies in
poison and never in another block's payload.  A kernel with such a defect therefore returns poison or leaves a
clobbered guard, and touches no memory the test does not own.  tests/test_far_ref.py checks all of this on the
CPU for every plan tests/test_gpu_far_strides.py uses.

Strides (elements):
  far_channel_stride  the smallest stride S with (C-1)·S past 2^31 elements and S·es past 2^32 bytes, plus a pad
                      longer than one channel: C = 2 fp32 -> 2^31 + pad, C = 3 fp32 -> 2^30 + pad (channel 1 past
                      2^32 bytes, channel 2 past 2^31 elements), C = 2 uint8 -> 2^32 + pad.  8-byte elements (the
                      fp64 state of rti_fit_accumulate) pass the byte limit only: 2^29 + pad; 2^31 doubles are
                      16 GiB per channel, beyond the memory cap once the base absorbs a signed truncation.
  far_row_stride      the smallest stride L with (n-1)·L past both limits for n rows (light planes, operator rows,
                      output rows), so the last row passes both and rows from about n/2 on pass the byte limit
                      (4-byte elements) or the element limit (uint8).
Both come `aligned` (multiples of the 16-byte vector: the predicates of rti_stack.h hold) and `odd` (aligned + 1:
one element per lane)."""
import numpy as np

from stride_ref import GUARD

LIM_ELEMS = 1 << 31
LIM_BYTES = 1 << 32
CAP_BYTES = 24 << 30  # no test holds more device memory than this at once
VARIANTS = ("aligned", "odd")


def u32(x):
    return int(x) & 0xFFFFFFFF


def s32(x):
    return ((int(x) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def truncations(e, es):
    """the four element offsets a 32-bit truncation of element offset e (element size es) can produce"""
    return (u32(e), s32(e), u32(e * es) // es, s32(e * es) // es)


def _up(x, m):
    return -(-int(x) // m) * m


def far_channel_stride(es, C, extent, variant="aligned"):
    """channel stride over `C` channels whose payload spans `extent` elements each"""
    vec = 16 // es if es <= 4 else 4
    need = max(-(-LIM_ELEMS // (C - 1)) if es <= 4 else 0, LIM_BYTES // es)
    return _up(need, vec) + _up(extent, vec) + vec + (variant == "odd")


def far_row_stride(es, n, extent, variant="aligned"):
    """row stride over `n` rows of `extent` elements each: the last row passes both limits"""
    vec = 16 // es if es <= 4 else 4
    need = max(LIM_ELEMS if es <= 4 else 0, LIM_BYTES // es)
    return _up(-(-need // (n - 1)), vec) + _up(extent, vec) + vec + (variant == "odd")


class Plan:
    def __init__(self, name, es, counts, strides, inner, far, guard=GUARD):
        self.name, self.es, self.far = name, int(es), int(far)  # strides[far] is the far one
        self.counts, self.strides = tuple(int(c) for c in counts), tuple(int(s) for s in strides)
        self.inner = int(inner)
        lo, hi = 0, 0
        for e in self.corner_offsets():
            t = truncations(e, self.es)
            lo, hi = min(lo, *t), max(hi, e, *t)
        align = max(16 // self.es, 1)
        self.base = _up(guard - lo, align)  # a 16-byte aligned payload base, `guard` elements before anything
        self.length = _up(self.base + hi + 1 + guard, align)

    def block_offsets(self):
        """true element offset, from the entry's pointer, of every block's first element: array of shape counts"""
        off = np.zeros((), np.int64)
        for n, s in zip(self.counts, self.strides):
            off = off[..., None] + np.arange(n, dtype=np.int64) * s
        return off

    def corner_offsets(self):
        """first and last element of every block"""
        first = self.block_offsets().ravel()
        return [int(e) for e in np.concatenate([first, first + self.inner - 1])]

    def in_payload(self, e):
        """is element offset e (from the pointer) part of some block"""
        first = self.block_offsets().ravel()
        return bool(((first <= e) & (e < first + self.inner)).any())

    def nbytes(self):
        return self.length * self.es

    def describe(self):
        rows = [f"{self.name}: es={self.es} counts={self.counts} strides={self.strides} inner={self.inner} "
                f"base={self.base} length={self.length} ({self.nbytes() / 2**30:.2f} GiB)"]
        for e in self.block_offsets().ravel():
            rows.append(f"  block at {int(e)} elements = {int(e) * self.es} bytes -> truncations "
                        f"{truncations(int(e), self.es)}")
        return "\n".join(rows)


def channel_plan(name, es, C, rows, inner, variant="aligned", row_stride=None):
    """C channels of `rows` dense rows (row stride `inner` unless given), the channels a far stride apart"""
    rs = inner if row_stride is None else row_stride
    return Plan(name, es, (C, rows), (far_channel_stride(es, C, rows * rs, variant), rs), inner, 0)


def row_plan(name, es, rows, inner, variant="aligned", C=1):
    """`rows` rows a far stride apart; C > 1 stacks dense channels (channel stride rows·L) behind each other"""
    L = far_row_stride(es, rows, inner, variant)
    return Plan(name, es, (C, rows), (rows * L, L), inner, 1)


# ---- the plans of tests/test_gpu_far_strides.py ---------------------------------------------------------------------
P0 = 1024 + 256 + 36  # the shapes of tests/test_gpu_strides.py
P16 = 1024 + 256 + 32  # q8 / h16, and 16 uint8 pixels per lane
ES = {"f32": 4, "i32": 4, "u8": 1}


def _plans():
    """name -> Plan.  The GPU module takes its plans from here by name and nowhere else, so test_far_ref.py sees each.

    farlight over 4-byte elements holds ONE channel: a second one must start at N·L >= 2^31 elements and end past
    2^32, which with the 2^31 elements in front of the base (the signed truncation of the first offset past 2^31)
    is 26 GiB, over the cap.  A single channel never uses its channel stride; farchan drives that.  uint8 stacks
    keep two channels, and the three of photometric stereo (ps-farlight-es1: 20 planes 2^32/19 bytes apart per
    channel, 14.4 GiB); its 4-byte farlight plans hold one channel for the same reason."""
    out = {}

    def add(p):
        assert p.name not in out, p.name
        out[p.name] = p

    for v in VARIANTS:
        # stacks: fp32 / int32 at P0 (N = 37 for the fit and fit + residual, 20 elsewhere); uint8 also at P16
        # (N = 37: 16 pixels per lane in rti_fit_shared; N = 20: q8 / h16)
        for es, N, P in ((4, 37, P0), (4, 20, P0), (1, 37, P0), (1, 20, P0), (1, 37, P16), (1, 20, P16)):
            add(channel_plan(f"stack-farchan-es{es}-N{N}-P{P}-{v}", es, 2, N, P, v))
            add(row_plan(f"stack-farlight-es{es}-N{N}-P{P}-{v}", es, N, P, v, C=2 if es == 1 else 1))
        for k, P in ((6, P0), (9, P0), (16, P0), (6, P16), (16, P16)):
            add(channel_plan(f"coef-farchan-k{k}-P{P}-{v}", 4, 2, 1, P * k, v))
        for k in (6, 16):
            add(channel_plan(f"state-farchan-k{k}-{v}", 8, 2, k + 1, P0, v))
        for E in (3, 257):
            add(channel_plan(f"opout-farchan-E{E}-{v}", 4, 2, E, P0, v))
        add(row_plan(f"opout-farrow-E3-{v}", 4, 3, P0, v))
        add(row_plan(f"op-farrow-N20-E3-{v}", 4, 20, 3, v))
        add(row_plan(f"cam-farlight-N50-P1024-{v}", 1, 50, 1024, v))
        add(channel_plan(f"pm-farchan-es4-N20-{v}", 4, 2, 1, P0 * 20, v))
        add(row_plan(f"pm-farpixel-es4-N20-{v}", 4, P0, 20, v))  # P0 pixel rows of N samples, one channel (as farlight)
        for k in (6, 9, 16):  # 1076 = 1024 + 52: the ragged size of the map readers' path tests
            add(channel_plan(f"maps-farchan-k{k}-P1076-{v}", 4, 3, 1, 1076 * k, v))
        for k in (6, 9, 16):  # 703 = 19 × 37: the multi-light image, 3 × 5 tiles of edge 8 ragged both ways
            add(channel_plan(f"maps-farchan-k{k}-P703-{v}", 4, 3, 1, 703 * k, v))
        # photometric stereo, N = 20 at P0.  farchan: three channels (4-byte: channel 1 past 2^32 bytes, channel 2 past
        # 2^31 elements; uint8: 2^32 and 2^33), the uint8 planes 1328 = 83·16 apart so that every plane of the aligned
        # variant starts on a 16-byte boundary and the tile is staged by 16-byte loads.  farlight: one channel of 4-byte
        # elements (the memory argument above), three of uint8 (14.4 GiB).
        add(channel_plan(f"ps-farchan-es4-N20-P{P0}-{v}", 4, 3, 20, P0, v))
        add(channel_plan(f"ps-farchan-es1-N20-P{P0}-{v}", 1, 3, 20, P0, v, row_stride=_up(P0, 16)))
        add(row_plan(f"ps-farlight-es4-N20-P{P0}-{v}", 4, 20, P0, v))
        add(row_plan(f"ps-farlight-es1-N20-P{P0}-{v}", 1, 20, P0, v, C=3))
    return out


PLANS = _plans()
