"""Strided views for the stack entries of include/rti.h, built on the host: a dense array embedded in a larger,
poisoned 1-D allocation, the index of every payload element, and the check that nothing but the payload changed.

A `Blocks` describes nested blocks in a flat buffer of `size` elements: element (i0, i1, .., j) of the payload,
i_d < counts[d] and j < inner, sits at start + Σ_d i_d·strides[d] + j.  Everything else is poison (inputs) or
guard (outputs).  Inputs are poisoned with a value the kernels cannot mistake for data (NaN / INT32_MIN / 255),
outputs are filled with NaN and compared as int32 bit patterns, so a written NaN of another payload is seen too.

tests/test_stride_ref.py checks this module without a GPU; tests/test_gpu_strides.py drives the entries with it."""
import numpy as np

NAN_BITS = np.int32(0x7FC00000)  # the float32 quiet NaN the output buffers are filled with
GUARD = 64  # elements before the first and after the last output block
POISON = {np.dtype(np.float32): np.float32(np.nan), np.dtype(np.int32): np.iinfo(np.int32).min,
          np.dtype(np.uint8): np.uint8(255)}

# the three stride / offset forms every entry is driven with: (lpad, cpad, opad, off, ooff), in elements; `vec` = 4 for fp32 / int32
# stacks, 16 for uint8 stacks (the aligned form keeps every 16-byte predicate of rti_stack.h true)
FORMS = ("aligned", "oddlight", "offset")


def form_pads(form, vec=4):
    if form == "aligned":
        return dict(lpad=vec, cpad=2 * vec, opad=4, off=0, ooff=0)
    if form == "oddlight":
        return dict(lpad=1, cpad=0, opad=0, off=0, ooff=0)
    if form == "offset":
        return dict(lpad=0, cpad=3, opad=2, off=1, ooff=1)
    raise ValueError(form)


class Blocks:
    def __init__(self, counts, strides, inner, start, size):
        self.counts, self.strides = tuple(int(c) for c in counts), tuple(int(s) for s in strides)
        self.inner, self.start, self.size = int(inner), int(start), int(size)
        assert len(self.counts) == len(self.strides)
        idx = self.index()
        assert idx.min() >= 0 and idx.max() < self.size, "payload outside the buffer"
        assert np.unique(idx).size == idx.size, "payload blocks overlap"

    def index(self):
        """int64 flat index of every payload element, shape counts + (inner,)"""
        idx = np.full((), self.start, np.int64)
        for n, s in zip(self.counts, self.strides):
            idx = idx[..., None] + np.arange(n, dtype=np.int64) * s
        return idx[..., None] + np.arange(self.inner, dtype=np.int64)

    def payload_mask(self):
        m = np.zeros(self.size, bool)
        m[self.index().ravel()] = True
        return m

    def gather(self, buf):
        return np.asarray(buf).reshape(-1)[self.index()]


def embed_stack(dense, lpad=0, cpad=0, off=0, poison=None, tail=GUARD):
    """dense [C, N, P] -> (buf, blocks, ls, cs): plane n of channel c at off + c·cs + n·ls with ls = P + lpad,
    cs = N·ls + cpad; every other element of buf (the first `off`, the pads, `tail` elements at the end) is poison."""
    dense = np.asarray(dense)
    C, N, P = dense.shape
    ls = P + lpad
    cs = N * ls + cpad
    b = Blocks((C, N), (cs, ls), P, off, off + C * cs + tail)
    buf = np.full(b.size, POISON[dense.dtype] if poison is None else poison, dense.dtype)
    buf[b.index()] = dense
    return buf, b, ls, cs


def out_blocks(C, block, pad=0, off=0, guard=GUARD):
    """C output blocks of `block` elements at guard + off + c·(block + pad), `guard` elements after the last"""
    ocs = block + pad
    start = guard + off
    return Blocks((C,), (ocs,), block, start, start + (C - 1) * ocs + block + guard), ocs


def out_rows(C, E, P, rpad=0, cpad=0, off=0, guard=GUARD):
    """C·E output rows of P elements: row e of channel c at guard + off + c·ocs + e·orow, orow = P + rpad,
    ocs = E·orow + cpad -> (blocks, orow, ocs)"""
    orow = P + rpad
    ocs = E * orow + cpad
    start = guard + off
    return Blocks((C, E), (ocs, orow), P, start, start + (C - 1) * ocs + (E - 1) * orow + P + guard), orow, ocs


def nan_buffer(blocks, dtype=np.float32):
    """the output buffer of `blocks`: every element the NaN bit pattern (as float32 or as int32)"""
    return np.full(blocks.size, NAN_BITS, np.int32).view(dtype)


def clobbered(buf, blocks, bits=NAN_BITS):
    """flat indices outside the payload whose 32-bit pattern is no longer `bits` (guards and gaps)"""
    raw = np.ascontiguousarray(buf).reshape(-1).view(np.int32)
    assert raw.size == blocks.size
    return np.flatnonzero((raw != bits) & ~blocks.payload_mask())


def untouched(buf, bits=NAN_BITS):
    """every element of an output buffer still holds `bits`: the entry wrote nothing at all"""
    return bool((np.ascontiguousarray(buf).reshape(-1).view(np.int32) == bits).all())
