"""trgt_plot_align_batch on the GPU, through the C ABI and trgt_amd/plot.py: every output of every designed case of tests/plot_cases.py, both
modes, equal to tests/pytrvz.py on the oracle's answers with no tolerance -- segments, counts, beta_proj, score, order --; host and device
blobs and outputs; every refusal with the outputs untouched; the context shared with trgt_locus_batch; a seeded fuzz."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plot_cases as pc  # noqa: E402
import pytrvz  # noqa: E402

pytestmark = pytest.mark.gpu
I32_MIN = -2147483648


@pytest.fixture(scope="module")
def ctx():
    from trgt_amd import _lib
    return _lib.context()


def run(ctx, mode, panels, **kw):
    from trgt_amd import plot
    b = plot.pack(mode, panels)
    outs = plot.alloc_outputs(b, fill=0xA5)
    plot.call(b, outs, ctx, **kw)
    return b, outs, plot.unpack(b, outs)


def want_of(mode, panel):
    if mode == 0:
        return pytrvz.get_allele_align(panel["motifs"], panel["lf"], panel["rf"], panel["ref"], panel["reads"], pc.hmm_oracle, pc.wfa_oracle)
    r = pytrvz.waterfall_align(panel["motifs"], panel["lf"], panel["rf"], panel["reads"], pc.hmm_oracle, pc.wfa_oracle)
    return dict(seq=None, reads=r["reads"], order=r["order"], scores=None)


def same(name, mode, got, want, n_reads):
    assert got["order"] == want["order"], (name, got["order"], want["order"])
    if mode == 0:
        assert got["seq"] == want["seq"], (name, got["seq"], want["seq"])
        assert got["scores"] == want["scores"], (name, got["scores"], want["scores"])
    else:
        assert got["scores"] == [I32_MIN] * n_reads, name
    assert len(got["reads"]) == len(want["reads"]) == n_reads
    for k, ((g_align, g_betas), (w_align, w_betas)) in enumerate(zip(got["reads"], want["reads"])):
        assert g_align == w_align, (name, "read drawn %d" % k, g_align, w_align)
        assert g_betas == w_betas, (name, "read drawn %d" % k, g_betas, w_betas)


@pytest.fixture(scope="module")
def designed(ctx):
    """both batches of designed cases, run once: mode -> (cases, packed batch, outputs, unpacked)"""
    res = {}
    for mode in (0, 1):
        cs = [c for c in pc.cases() if c["mode"] == mode]
        res[mode] = (cs,) + run(ctx, mode, [c["panel"] for c in cs])
    return res


@pytest.mark.parametrize("mode", [0, 1])
def test_designed_cases(designed, mode):
    cs, b, outs, got = designed[mode]
    assert len(cs) >= 5
    for c, g in zip(cs, got):
        same(c["name"], mode, g, pc.expected(c), len(c["panel"]["reads"]))
    # segment counts stay inside trgt_plot_seg_capacity, and a host array is written in the used part of every slot only
    for r in range(len(b["read_len"])):
        o, e, n = int(b["rseg_off"][r]), int(b["rseg_off"][r + 1]), int(outs["n_rseg"][r])
        assert n <= e - o
        assert (outs["rseg"][2 * (o + n):2 * e] == 0xA5A5A5A5).all(), r
    for p in range(b["n_panels"] if mode == 0 else 0):
        o, e, n = int(b["pseg_off"][p]), int(b["pseg_off"][p + 1]), int(outs["n_pseg"][p])
        assert n <= e - o and (outs["pseg"][2 * (o + n):2 * e] == 0xA5A5A5A5).all(), p


def test_every_case_alone_gives_what_it_gives_in_the_batch(ctx, designed):
    # (a batch of one panel: other launch classes, other slot offsets)
    for mode in (0, 1):
        cs, _, _, got = designed[mode]
        for c, g in list(zip(cs, got))[::4]:
            _, _, alone = run(ctx, mode, [c["panel"]])
            assert alone[0] == g, c["name"]


def test_host_and_device_blobs_and_outputs_give_the_same(ctx, designed):
    import torch
    from trgt_amd import plot
    for mode in (0, 1):
        cs, b, outs, got = designed[mode]
        ref_dev, read_dev = torch.from_numpy(b["ref_blob"]).cuda(), torch.from_numpy(b["read_blob"]).cuda()
        outs2 = plot.alloc_outputs(b, fill=0xA5)
        plot.call(b, outs2, ctx, ref_blob=ref_dev, read_blob=read_dev)
        assert plot.unpack(b, outs2) == got
        dev = {k: torch.from_numpy(v).cuda() for k, v in plot.alloc_outputs(b, fill=0xA5).items()}
        plot.call(b, dev, ctx, ref_blob=ref_dev, read_blob=read_dev)
        torch.cuda.synchronize()
        assert plot.unpack(b, {k: v.cpu().numpy() for k, v in dev.items()}) == got
        # the optional outputs left out
        outs3 = plot.alloc_outputs(b, fill=0xA5)
        some = {k: v for k, v in outs3.items() if k not in ("beta_proj", "score", "order")}
        plot.call(b, some, ctx)
        for k in ("pseg", "n_pseg") if mode == 0 else ():
            assert (outs3[k] == outs[k]).all()
        assert (outs3["n_rseg"] == outs["n_rseg"]).all() and (outs3["rseg"] == outs["rseg"]).all()


def test_no_betas_at_all(ctx, designed):
    from trgt_amd import plot
    cs, b, outs, got = designed[0]
    b2 = dict(b, beta_begin=None, beta_pos=None)
    outs2 = plot.alloc_outputs(b, fill=0xA5)
    plot.call(b2, outs2, ctx)
    assert (outs2["rseg"] == outs["rseg"]).all() and (outs2["n_rseg"] == outs["n_rseg"]).all() and (outs2["score"] == outs["score"]).all()
    assert (outs2["beta_proj"].view(np.uint8) == 0xA5).all()


def small_panel():
    c = next(c for c in pc.cases() if c["name"] == "convert_boundaries")
    p = c["panel"]
    return dict(p, reads=p["reads"][:3])


ERRORS = {
    "mode": (lambda b: b.update(mode=2), -1, "mode 2"),
    "null_ref_len": (lambda b: b.update(ref_len=None), -1, "null field"),
    "null_read_off": (lambda b: b.update(read_off=None), -1, "null field"),
    "panel_set": (lambda b: b["panel_set"].__setitem__(0, 1), -1, "panel 0 has motif set 1 of 1"),
    "panel_read_begin": (None, -1, "panel_read_begin decreases at panel 1"),   # (two panels, below)
    "ref_len_short": (lambda b: b["ref_len"].__setitem__(0, 99), -1, "panel 0 has ref_len 99"),
    "byte_read": (lambda b: b["read_blob"].__setitem__(int(b["read_off"][1]) + 4, ord("N")), -1, "read 1 has byte 0x4e at position 4"),
    "byte_ref": (lambda b: b["ref_blob"].__setitem__(7, ord("a")), -1, "the reference of panel 0 has byte 0x61 at position 7"),
    "byte_motif": (lambda b: b["motif_blob"].__setitem__(8, ord("X")), -1, "motif 1 of set 0 has byte 0x58"),
    "beta_order": (lambda b: b["beta_pos"].__setitem__(1, int(b["beta_pos"][0])), -1, "the betas of read 0 are not strictly increasing"),
    "beta_range": (lambda b: b["beta_pos"].__setitem__(int(b["beta_begin"][1]) - 1, int(b["read_len"][0])), -1, "read 0 has a beta at position"),
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_refused_with_outputs_untouched(ctx, name):
    from trgt_amd import _lib, plot
    change, code, text = ERRORS[name]
    b = plot.pack(0, [small_panel()])
    if name == "panel_read_begin":   # (needs a second panel)
        b = plot.pack(0, [small_panel(), small_panel()])
        b["panel_read_begin"] = np.array([0, 4, 3], np.uint64)
    else:
        change(b)
    outs = plot.alloc_outputs(plot.pack(0, [small_panel(), small_panel()]), fill=0xA5)
    rc = plot.call(b, outs, ctx, check=False)
    msg = _lib.lib().trgt_hip_last_error(ctx.handle).decode()
    assert rc == code, (rc, msg)
    assert text in msg, msg
    for k, v in outs.items():
        assert (v.view(np.uint8) == 0xA5).all(), k


def test_mode1_refusals_and_model_limit(ctx):
    from trgt_amd import _lib, plot
    p = next(c for c in pc.cases() if c["name"] == "waterfall_a")["panel"]

    def refused(b, code, text):
        outs = plot.alloc_outputs(b, fill=0xA5)
        rc = plot.call(b, outs, ctx, check=False)
        msg = _lib.lib().trgt_hip_last_error(ctx.handle).decode()
        assert rc == code and text in msg, (rc, msg)
        for k, v in outs.items():
            assert (v.view(np.uint8) == 0xA5).all(), k
    # a waterfall reference is exactly the two flanks
    b = plot.pack(1, [dict(p, ref=p["lf"] + "A" + p["rf"])])
    refused(b, -1, "panel 0 has ref_len 101")
    # a read shorter than its flanks: the reference's slice panics there
    b = plot.pack(1, [dict(p, reads=[p["reads"][0], dict(seq=(p["lf"] + p["rf"])[:99], betas=[])])])
    refused(b, -1, "read 1 of panel 0 has 99 bases")
    # a motif set beyond the HMM's 4 096 states, worded as trgt_hmm_batch words it
    rng = random.Random(5)
    big = ["".join(rng.choice("ACGT") for _ in range(700)) for _ in range(2)]
    b = plot.pack(1, [dict(p, motifs=big)])
    refused(b, -3, "trgt_hmm_batch: set 0 has 4209 HMM states")
    # ... and beyond 253 motifs
    b = plot.pack(1, [dict(p, motifs=["ACG"] * 254)])
    refused(b, -3, "too many motifs")


def test_context_shared_with_trgt_locus_batch(ctx, designed):
    """WfaOnDevice and the HMM buffers are the context's: a plot call between two locus calls, and the other way round"""
    from trgt_amd import locus, synth
    b = synth.generate(6, first_locus=7)
    keys = ("span_start", "span_end", "n_alleles", "allele_len", "allele_blob", "ci", "purity", "n_spans", "spans3", "motif_counts")
    first = locus.run_batch(b, ctx=ctx)
    before = {k: np.array(getattr(first, k), copy=True) for k in keys}
    cs, _, _, got = designed[0]
    _, _, again = run(ctx, 0, [c["panel"] for c in cs])
    assert again == got
    second = locus.run_batch(b, ctx=ctx)
    for k in keys:
        a, c2 = before[k], np.asarray(getattr(second, k))
        assert a.tobytes() == c2.tobytes(), k
    cs1, _, _, got1 = designed[1]
    _, _, again1 = run(ctx, 1, [c["panel"] for c in cs1])
    assert again1 == got1


def test_kernel_times_are_reported(ctx, designed):
    from trgt_amd import plot
    cs, _, _, _ = designed[0]
    ctx.timing_enable(True)
    try:
        run(ctx, 0, [c["panel"] for c in cs[:4]])
        ms = plot.kernel_ms(ctx)
    finally:
        ctx.timing_enable(False)
    assert ms[0] > 0.0 and ms[1] > 0.0, ms
    run(ctx, 0, [cs[0]["panel"]])
    assert plot.kernel_ms(ctx) == (0.0, 0.0)


# ---- a seeded fuzz: 40 panels x 8 reads, flanks of 50, alleles of 0 to 300 bases over 1 to 3 motifs, reads through a local error channel,
#      random strictly increasing betas, both modes
def noisy(rng, seq, rate):
    out = []
    for ch in seq:
        u = rng.random()
        if u < rate:
            out.append(rng.choice("ACGT"))          # substitution (or, one time in four, none)
        elif u < 1.6 * rate:
            continue                                # deletion
        elif u < 2.2 * rate:
            out.append(ch)
            out.append(rng.choice("ACGT"))          # insertion
        else:
            out.append(ch)
    return "".join(out)


def fuzz_panels(seed, mode):
    rng = random.Random(seed)
    panels = []
    for p in range(40):
        motifs = []
        while len(motifs) < rng.randint(1, 3):
            m = "".join(rng.choice("ACGT") for _ in range(rng.choice([1, 2, 3, 3, 4, 5, 6, 7, 9, 12])))
            if m not in motifs:
                motifs.append(m)
        lf, rf = pc.rand_seq(rng, 50), pc.rand_seq(rng, 50)
        target = rng.choice([0, 0, 5, 30, 60, 100, 200, 300])
        allele = ""
        while len(allele) < target:
            allele += rng.choice(motifs) * rng.randint(1, 6)
        allele = noisy(rng, allele[:target], 0.03)
        ref = lf + allele + rf
        reads = []
        for _ in range(8):
            rate = rng.choice([0.0, 0.01, 0.03, 0.06])
            if mode == 0:
                seq = noisy(rng, ref, rate) or "A"
            else:   # the read's flanks are cut by length: keep them as long as the locus's
                seq = (noisy(rng, lf, rate) + lf)[:50] + noisy(rng, allele, rate) + (rf + noisy(rng, rf, rate))[-50:]
            n = rng.choice([0, 0, 1, 3, 10, 70])
            pos = sorted(rng.sample(range(len(seq)), min(n, len(seq))))
            reads.append(dict(seq=seq, betas=[(q, round(rng.random(), 6)) for q in pos]))
        panels.append(dict(motifs=motifs, lf=lf, rf=rf, ref=ref if mode == 0 else lf + rf, reads=reads))
    return panels


@pytest.mark.parametrize("mode", [0, 1])
def test_fuzz(ctx, mode):
    panels = fuzz_panels(1234 + mode, mode)
    _, _, got = run(ctx, mode, panels)
    for i, (p, g) in enumerate(zip(panels, got)):
        same("fuzz panel %d" % i, mode, g, want_of(mode, p), 8)
