"""Models that carry a chroma mix, and the pictures the two list calls with a model per picture must make of them (TEST INFRASTRUCTURE;
include/vfgs_hip.h "models that carry a mix", include/vfgs_hip_fw.h vfgs_hip_models_from_afgs1_mix).

A model here is a recorded AFGS1 parameter set (tests/golden/fwcfg, with the reference firmware's programming of it in tests/golden/traces)
whose mix fields are ALTERED, so that the models of a list differ in their mix:

    luma_only   cb_mult / cb_luma_mult / cb_offset = 128 / 192 / 256, what every .cfg of the reference says: (64, 0, 0)
    tbl         fgs_afgs1_test1.tbl's 247 192 18 / 229 182 54
    cfl         chroma_scaling_from_luma = 1: (64, 0, 0), and Cb and Cr take the luma scaling function
    neutral     192 / 128 / 256: (0, 64, 0), the chroma sample itself
    cb_only     a mix on Cb alone -- no parameter set gives that: programmed with vfgs_hip_set_chroma_mix and captured
    none        no mix: vfgs_hip_models_from_afgs1

Only one parameter set is recorded at 4:4:4 and one at 4:2:2, so the models of those cases are told apart by more than their mix through
two further alterations, each with programming that is one altered record of the recorded trace (vfgs_fw.c's vfgs_set_scale_shift(
grain_scaling - 6) and vfgs_set_legal_range(clip_to_restricted_range)), written "+full" / "+shift" behind the kind:

    +full       clip_to_restricted_range = 0 (the recorded sets at 4:4:4 and 4:2:2 say 1): the record's clip bounds are the full range's
    +shift      grain_scaling one higher: the record's scale shift differs

With cfl (another chroma scale LUT, hence another IMAGE) a frame's image, bounds and shift each differ from those of the launch's first frame.

The contract is the loop of the list call -- program the state models[f] was captured from, ITS MIX INCLUDED; with seeds vfgs_set_seed(seeds[f]);
grain frame f -- so the expectation is tests/model_list_util.py's seed handling (a context per model reseeded per frame, or one context into
which the frame's program is replayed without its seed) around tests/chroma_mix_util.py's derivation (the unchanged oracle on the index frame),
per frame, with that frame's records and that frame's mix.  Samples on a clip bound are left out by that derivation and counted."""
import chroma_mix_util as X
import model_list_util as U
import semiplanar_util as SP
import vfgs_testlib as T

KINDS = ("luma_only", "tbl", "cfl", "neutral", "cb_only", "none")
TBL = ((247, 192, 18), (229, 182, 54))      # (mult, luma_mult, offset) of Cb, of Cr


def base(kind):
    return kind.split("+")[0]


def flags(kind):
    return set(kind.split("+")[1:])


def fields(kind):
    """(cb_mult, cb_luma_mult, cb_offset), (cr_...) written into the parameter set"""
    kind = base(kind)
    return {"luma_only": ((128, 192, 256),) * 2, "tbl": TBL, "neutral": ((192, 128, 256),) * 2}.get(kind, ((128, 192, 256),) * 2)


def mix_of(kind):
    """(mix of Cb, mix of Cr) the model carries, each (luma_mult, chroma_mult, offset) or None, as vfgs_init_afgs1 derives them"""
    kind = base(kind)
    if kind == "none":
        return (None, None)
    if kind == "cfl":
        return ((64, 0, 0),) * 2
    if kind == "cb_only":
        return ((24, 40, 3), None)
    return tuple((lm - 128, m - 128, off - 256) for m, lm, off in fields(kind))


def parameter_set(name, kind):
    """the recorded parameter set `name` with the mix fields of `kind`"""
    from versatilefilmgrain_amd import fw
    raw = T.load_fwcfg(name)[1][-1]
    assert raw[0] == 1
    a = fw.struct_from_bytes(1, raw[1])
    (a.cb_mult, a.cb_luma_mult, a.cb_offset), (a.cr_mult, a.cr_luma_mult, a.cr_offset) = fields(kind)
    a.chroma_scaling_from_luma = 1 if base(kind) == "cfl" else 0
    if "full" in flags(kind):
        assert a.clip_to_restricted_range == 1
        a.clip_to_restricted_range = 0
    if "shift" in flags(kind):
        a.grain_scaling += 1
    return a


def records(name, kind):
    """the oracle's programming of parameter_set(name, kind): the recorded one; cfl: Cb's and Cr's scale LUTs are luma's (vfgs_fw.c:676-682)"""
    rec = U.model_records(name)
    if "full" in flags(kind):
        assert [a for op, a, *_ in rec if op == T.OP_LEGAL_RANGE] == [1]
        rec = [(op, 0, b, p) if op == T.OP_LEGAL_RANGE else (op, a, b, p) for op, a, b, p in rec]
    if "shift" in flags(kind):      # (the firmware sets the shift twice, to the same value)
        assert len({a for op, a, *_ in rec if op == T.OP_SCALE_SHIFT}) == 1
        rec = [(op, a + 1, b, p) if op == T.OP_SCALE_SHIFT else (op, a, b, p) for op, a, b, p in rec]
    if base(kind) != "cfl":
        return rec
    luma = [p for op, a, _b, p in rec if op == T.OP_SCALE_LUT and a == 0][-1]
    return [(op, a, b, luma) if (op == T.OP_SCALE_LUT and a in (1, 2)) else (op, a, b, p) for op, a, b, p in rec]


def expect_list(models, pick, frames, seeds, ora=None):
    """models: [(records, mixes)]; frames: planar T.Frames.  seeds given: a context per model, reseeded per frame; else ONE context (`ora`, or
    one programmed with the last model's records) into which the frame's program is replayed without its seed.
    -> ([(expected, masks)], excluded samples, the four registers afterwards, the context of an unseeded run)"""
    res, excluded = [], 0
    if seeds is not None:
        oras = [U.oracle_programmed(r) for r, _ in models]
    else:
        ora = ora or U.oracle_programmed(models[-1][0])
    for i, (f, k) in enumerate(zip(frames, pick)):
        rec, mixes = models[k]
        if seeds is not None:
            o = oras[k]
            o.set_seed(seeds[i])
        else:
            o = ora
            T.replay(o, U.without_seed(rec))
        fi = X.index_frame(f, mixes)
        out = fi.copy()
        o.add_grain_frame(out)
        want, masks, ex = X.expect_from(f, fi, out, X.legal_range(rec))
        res.append((want, masks))
        excluded += ex
    return res, excluded, (oras[pick[-1]] if seeds is not None else ora).seed_state(), ora


def to_sp_expectation(sp, want, masks):
    """a planar expectation of D(sp) written over a copy of the semi-planar source where the call writes (tests/semiplanar_mix_util.py) -> (SPFrame, UV mask)"""
    import numpy as np
    rows, crows, cols = SP.written_region(sp)
    w = sp.copy()
    w.Y[:rows, :cols] = want.Y[:rows, :cols] << sp.shift
    w.UV[:crows, 0:cols:2] = want.U[:crows, :cols // 2] << sp.shift
    w.UV[:crows, 1:cols:2] = want.V[:crows, :cols // 2] << sp.shift
    m = np.ones(sp.UV.shape, bool)
    m[:crows, 0:cols:2] = masks[0][:crows, :cols // 2]
    m[:crows, 1:cols:2] = masks[1][:crows, :cols // 2]
    return w, m


# ---- the case table: what tests/test_gpu_model_list_mix.py runs on the GPU and tests/test_model_mix_cases_cpu.py holds to 0 excluded samples

# content: luma over [0.3, 0.7) of the range; chroma inside it, narrowed where a mix with a large chroma multiplier (the .tbl's 119 / 64
# and 101 / 64 with offsets of -238 and -202) would otherwise push the index onto 0 or 2^depth - 1
CONTENT = dict(lo=0.3, hi=0.7, clo=0.42, chi=0.5)

# id -> (parameter sets and kinds of models A, B, C; width, height)
PLANAR = {
    "10_420_1047x40": ([("fgs_afgs1_test1_10_420", "tbl"), ("fgs_afgs1_test9_10_420", "cfl"), ("fgs_afgs1_test3_10_420", "none")], 1047, 40),
    "8_444_183x33": ([("fgs_afgs1_test1_8_444", "tbl"), ("fgs_afgs1_test1_8_444", "cfl+full"), ("fgs_afgs1_test1_8_444", "none")], 183, 33),
    "10_422_200x48": ([("fgs_afgs1_test3_10_422", "cfl+full+shift"), ("fgs_afgs1_test3_10_422", "cb_only"), ("fgs_afgs1_test3_10_422", "none")], 200, 48),
}
# id -> (models A, B, C; width, height, sample_shift)
SEMIPLANAR = {
    "p010_1047x40": ([("fgs_afgs1_test1_10_420", "tbl"), ("fgs_afgs1_test9_10_420", "cfl"), ("fgs_afgs1_test3_10_420", "none")], 1047, 40, 6),
    "nv12_183x34": ([("fgs_afgs1_test1_8_420", "luma_only"), ("fgs_afgs1_test9_8_420", "tbl"), ("fgs_afgs1_test3_8_420", "none")], 183, 34, 0),
    "p210_200x48": ([("fgs_afgs1_test3_10_422", "tbl"), ("fgs_afgs1_test3_10_422", "cfl+full+shift"), ("fgs_afgs1_test3_10_422", "none")], 200, 48, 6),
}
PICK = [0, 1, 0, 2, 1]       # A B A C B
CYCLE = [("fgs_afgs1_test1_10_420", k) for k in ("luma_only", "tbl", "cfl", "neutral")]      # 34 frames, mixes cycling
CYCLE_SIZE = (136, 32)       # (the hardware layer refuses widths up to 128, vfgs_hw.c:168: nine blocks, the last ragged, by two block rows)


def case_models(spec):
    return [(records(n, k), mix_of(k)) for n, k in spec]


def case_frames(spec, width, height, n, seed):
    depth, sx, sy = T.trace_geometry(U.model_records(spec[0][0]))
    return X.ranged_frames(width, height, depth, sx, sy, n, seed, **CONTENT)


def fresh_seeds(n, seed):
    import numpy as np
    return [int(s) for s in np.random.default_rng(seed).integers(0, 1 << 32, n)]
