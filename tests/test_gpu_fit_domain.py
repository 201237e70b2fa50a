"""The shared-direction fits (rti_fit_shared, rti_fit_shared_pm) over their whole input domain, against
tests/fit_domain_ref.py: signed fractional, wide-range, full-range int32 and non-finite stacks.

Every assertion is one of three: |got − reference| <= the derived fp32 bound per coefficient (γ_{N+1} for the VALU
and lane kernels, γ_{2(N+1)} for the matrix-core kernels), bit equality with the exact fmaf chain (every VALU variant
of rti_fit_shared but the rotated measurement variant, and the one-lane-per-pixel pm fit), and equality of the
finite / +Inf / −Inf / NaN class of every coefficient of a poisoned stack.

One seeded stack per (basis, N) and class is made at the largest pixel count; every shape is its first P pixels, so
the reference and the exact chain are computed once and shared."""
import functools

import numpy as np
import pytest
import torch

import fit_domain_ref as fr
import rti

pytestmark = pytest.mark.gpu

L = rti._lib
TERMS = {"ptm": 6, "hsh9": 9, "hsh": 16}
CH, SP, DEPTH, WAVES = (L.RTI_KERNEL_CHUNKS_SHIFT, L.RTI_KERNEL_TILE_PLANES_SHIFT, L.RTI_KERNEL_TILE_DEPTH_SHIFT,
                        L.RTI_KERNEL_TILE_WAVES_SHIFT)
NT, LDSW, NTS, STAGE = L.RTI_KERNEL_NONTEMPORAL, L.RTI_KERNEL_PINV_LDS, L.RTI_KERNEL_NT_STORE, L.RTI_KERNEL_STAGE

# rti_fit_shared forms: name -> (kernel, flags, unit, exact).  `unit` is the form's wave or tile width in pixels
# (256 · chunks for the VALU stream, 256 · rc for the tiles); `exact`: held to valu_exact's bits where it runs VALU.
LM_FORMS = {}
for f in (0, NT, LDSW, NTS, STAGE, NT | LDSW | NTS | STAGE):
    LM_FORMS[f"valu-0x{f:03x}"] = ("valu", f, 256, True)
for c in (2, 3, 4, 8):
    LM_FORMS[f"valu-nt-chunks{c}"] = ("valu", NT | (c << CH), 256 * c, True)
LM_FORMS["auto-rotate-chunks4"] = ("auto", L.RTI_KERNEL_ROTATE | (4 << CH), 1024, False)  # another order: bound only
LM_FORMS["mfma"] = ("mfma", 0, 256, True)
LM_FORMS["mfma-nt"] = ("mfma", NT, 256, True)
for rc, sp, depth in ((1, 1, 2), (2, 2, 2), (4, 1, 3), (8, 2, 4)):
    LM_FORMS[f"tile-rc{rc}-sp{sp}-d{depth}"] = ("tile", (rc << CH) | (sp << SP) | (depth << DEPTH), 256 * rc, True)
for rc, depth in ((4, 2), (8, 3), (15, 1)):
    LM_FORMS[f"tile-w8-rc{rc}-d{depth}"] = ("tile", (rc << CH) | (depth << DEPTH) | (8 << WAVES), 256 * rc, True)
LM_FORMS["auto"] = ("auto", 0, 256, True)

LM_CASES = [(b, N) for b, k in TERMS.items() for N in [17, 23, 36, 38] + ([k + 1] if k in (6, 9) else [])]
PM_LIGHTS = (17, 20, 36, 100)
P_EXACT = 3 * 2048 + 272  # the widest shape held to exact bits (uint8 at 8 chunks)
P_MAX = 3 * 256 * 15 + 260  # the widest shape at all (the 8-wave tile at rc = 15)
P_PM = 1008  # the pixel-major shapes' pixels held to exact bits (P <= 1003)


def lm_family(kernel, P):
    """The kernel family rti_fit_shared runs for k in {6, 9, 16}: the MFMA and tile kernels need 4-pixel alignment
    and fall back to the one-chunk VALU stream without it; AUTO is the VALU stream below 2^21 pixels."""
    return "valu" if kernel in ("valu", "auto") or P % 4 else kernel


@functools.lru_cache(maxsize=2)
def case(basis, N):
    """(fp32 pseudo-inverse, stacks [2, N, P_MAX] by class)"""
    lu, lv = _dirs(N)
    w = rti.pinv(lu, lv, basis).astype(np.float32)
    return w, dict(fr.stacks(np.random.default_rng(100 * N + TERMS[basis]), 2, N, P_MAX))


@functools.lru_cache(maxsize=8)
def exact_bits(basis, N, name, pixels):
    """the exact VALU chain of the first `pixels` pixels of a class's stack: [2, pixels, k] fp32"""
    w, st = case(basis, N)
    return fr.valu_exact(w, st[name][:, :, :pixels])


def _dirs(N):
    import rti_oracle as o

    return o.synth_dirs(N, 11)


class Judge:
    """Collects every miss of a parametrised case, so that one run reports them all."""

    def __init__(self, what):
        self.what, self.misses, self.worst = what, [], {}

    def bound(self, tag, family, got, ref, bnd):
        ratio, at = fr.worst_ratio(got, ref, bnd)
        self.worst[family] = max(self.worst.get(family, 0.0), ratio)
        if not ratio <= 1:
            self.misses.append(f"{tag}: err/bound {ratio:.3g} at (c, p, k) = {at} [{family}]")

    def bits(self, tag, got, exact):
        same = got.view(np.int32) == exact.view(np.int32)
        if not same.all():
            at = tuple(int(i) for i in np.argwhere(~same)[0])
            self.misses.append(f"{tag}: {int((~same).sum())} of {same.size} coefficients differ from the exact fmaf "
                               f"chain, first at (c, p, k) = {at}: got {got[at]!r}, exact {exact[at]!r}")

    def classes(self, tag, got, want):
        have = fr.classify(got)
        if not np.array_equal(have, want):
            at = tuple(int(i) for i in np.argwhere(have != want)[0])
            self.misses.append(f"{tag}: {int((have != want).sum())} coefficients of another class "
                               f"(0 finite, 1 +inf, 2 -inf, 3 nan), first at (c, p, k) = {at}: got class {have[at]}, "
                               f"reference {want[at]}")

    def done(self):
        for family, ratio in sorted(self.worst.items()):
            print(f"WORST {family}: {ratio:.3f}  ({self.what})")
        assert not self.misses, f"{self.what}: {len(self.misses)} misses\n" + "\n".join(self.misses)


def _run(entry, pv, I, k, layout, **kw):
    """One launch on a NaN-filled output; the coefficients as [C, P, k] on the host."""
    C, P = (I.shape[0], I.shape[2]) if entry is rti.fit_shared_into else (I.shape[0], I.shape[1])
    coef = torch.full((C, P, k) if layout == "pixel" else (C, k, P), float("nan"), device=I.device)
    entry(pv, I, coef, k=k, layout=layout, **kw)
    got = coef.cpu().numpy()
    return got if layout == "pixel" else np.ascontiguousarray(np.moveaxis(got, 1, 2))


def _judge_stacks(judge, tag, run, family, exact_bits, w, named, exact):
    """`named`: (class name, host stack [C, N, P]) pairs; run(class name, host stack, layout) -> [C, P, k]"""
    roundings = 1 if family in ("valu", "lane", "pm-valu-stream") else 2
    for name, I in named:
        P = I.shape[2]
        ref, bnd = fr.reference(w, I), fr.bound(w, I, roundings)
        poisoned = name == "poisoned"
        for layout in ("pixel", "planar"):
            got = run(name, I, layout)
            t = f"{tag} P={P} {name} {layout}"
            if poisoned:
                judge.classes(t, got, fr.classify(ref))
            judge.bound(t, family, got, ref, bnd)  # of the coefficients whose reference is finite
            if exact_bits and not poisoned:
                judge.bits(t, got, exact(name)[:, :P])


def _poisoned(I):
    Ip = I.copy()
    fr.poison(Ip)
    return Ip


@pytest.mark.parametrize("form", list(LM_FORMS))  # varies fastest: a (basis, N) case's stacks are made once
@pytest.mark.parametrize("basis,N", LM_CASES)
def test_fit_shared_domain(cuda, basis, N, form):
    """rti_fit_shared: light counts with N % 4 = 1, 3, 0, 2 (a partial 16-light chunk, the MFMA kernel's 32-light main
    loop plus its tail) and N = k + 1; P = 259 (one pixel per lane) and three whole waves or tiles plus a ragged 260;
    two channels, both coefficient layouts, fp32 and int32 stacks, and uint8 for the VALU stream (16-pixel lanes for
    PTM-6 at a pixel count that is a multiple of 16)."""
    kernel, flags, unit, exact_ok = LM_FORMS[form]
    k = TERMS[basis]
    w, st = case(basis, N)
    exact = functools.partial(exact_bits, basis, N, pixels=P_EXACT)
    pv = torch.as_tensor(w, device=cuda)
    judge = Judge(f"rti_fit_shared {form} {basis} N={N}")

    def run(name, I, layout):
        return _run(rti.fit_shared_into, pv, torch.as_tensor(np.ascontiguousarray(I)).to(cuda), k, layout,
                    kernel=kernel, flags=flags)

    for P in (259, 3 * unit + 260):
        family = lm_family(kernel, P)
        named = [(name, st[name][:, :, :P]) for name in ("signed", "wide", "i32")]
        named.append(("poisoned", _poisoned(named[0][1])))
        _judge_stacks(judge, form, run, family, exact_ok and family == "valu", w, named, exact)
    if kernel == "valu":
        for P in (259, 3 * unit + 260, 3 * min(4 * unit, 2048) + 272):
            _judge_stacks(judge, form, run, "valu", True, w, [("u8", st["u8"][:, :, :P])], exact)
    judge.done()


# rti_fit_shared_pm forms: name -> (kernel, flags)
PM_FORMS = {
    "auto": ("auto", 0),
    "auto-stage": ("auto", STAGE),  # the direct form where N % 4 == 0
    "mfma-w3": ("mfma", 3 << WAVES),
    "mfma-w8": ("mfma", 8 << WAVES),
    "tile-g2-w2": ("tile", (2 << CH) | (2 << WAVES)),
    "valu": ("valu", 0),  # one lane per pixel
}
PM_FAMILY = {0: "lane", L.RTI_PM_VALU_STREAM: "pm-valu-stream", L.RTI_PM_MFMA_STREAM: "pm-mfma-stream",
             L.RTI_PM_BLOCK: "pm-block", L.RTI_PM_DIRECT: "pm-direct"}
PM_CASES = [("auto-ragged", 17)] + [(f, N) for N in PM_LIGHTS for f in PM_FORMS]


@pytest.mark.parametrize("form,N", PM_CASES)
@pytest.mark.parametrize("basis", list(TERMS))
def test_fit_shared_pm_domain(cuda, basis, form, N):
    """rti_fit_shared_pm on the same stacks, pixel-major: P = 68 and 1000, bumped until P·N % 4 == 0 where the form
    needs it (the DMA kernels), and for "auto-ragged" P = 67 and 1001 at N = 17, which AUTO hands to the lane
    kernel."""
    ragged = form == "auto-ragged"
    kernel, flags = ("auto", 0) if ragged else PM_FORMS[form]
    k = TERMS[basis]
    w, st = case(basis, N)
    exact = functools.partial(exact_bits, basis, N, pixels=P_PM)
    pv = torch.as_tensor(w, device=cuda)
    judge = Judge(f"rti_fit_shared_pm {form} {basis} N={N}")

    def run(name, I, layout):
        Ipm = torch.as_tensor(np.ascontiguousarray(np.swapaxes(I, 1, 2))).to(cuda)  # [C, P, N]
        return _run(rti.api.fit_shared_pm_into, pv, Ipm, k, layout, kernel=kernel, flags=flags)

    for P in (67, 1001) if ragged else (68, 1000):
        while kernel != "valu" and not ragged and (P * N) % 4:
            P += 1
        for dtype, names in ((L.RTI_F32, ("signed", "wide")), (L.RTI_I32, ("i32",))):
            plan = L.lib().rti_fit_shared_pm_plan(k, N, dtype, P, 2, 0, 0, flags | rti.api._KERNELS[kernel])
            if plan == 0 and kernel in ("mfma", "tile"):
                pytest.skip("plan does not fit the LDS")
            assert (plan == 0) == (ragged or kernel == "valu"), (plan, P)
            family = PM_FAMILY[plan // 10 ** 8]
            named = [(name, st[name][:, :, :P]) for name in names]
            if dtype == L.RTI_F32:
                named.append(("poisoned", _poisoned(named[0][1])))
            _judge_stacks(judge, f"{form} plan {plan}", run, family, family == "lane", w, named, exact)
    judge.done()
