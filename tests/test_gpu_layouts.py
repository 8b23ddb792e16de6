"""GPU (MI355X): the layout ledger -- every kernel key and every public entry that takes picture memory, on the memory a real caller hands
over.  The rest of the suite pins WHAT the kernels compute; every plane it passes is a torch allocation of its own (256-byte aligned, the
pitch rounded up to 64 samples, the height to 16 rows).  include/vfgs_hip.h promises more: pointers 16-byte aligned, pitches any multiple of
16 bytes that holds the whole blocks of a row, and no byte outside those blocks and no row outside the addressed lines written or relied on.

tests/layout_cases.py has the table (a case per line of tests/golden/kernel_keys.txt, and the entries of hw.VfgsHip with the host pipe),
tests/layout_arena.py the memory: ONE allocation per call that holds every plane back to back, bases 16 but never 256 aligned, the smallest
legal pitches, exactly the addressed rows (odd heights; a part's own lines only), random guards of at least 16 KiB in front, between and
behind.  tests/test_layout_cases_cpu.py checks table, layouts and comparison on the oracle alone.

A case resets the state, programs the model (the mix cleared in `finally`), uploads the arena, makes the call with pointers into it,
downloads it and compares the WHOLE arena with the expectation in one comparison -- under a mix the samples the derivation leaves out are
masked inside the region only --, then the four seed registers with the oracle's.  A key's case also asserts what
test_gpu_kernel_keys.check_launch asserts: the tight layout still ran THAT kernel.  Damage is found by comparing bytes, never by a fault."""
import ctypes as C

import numpy as np
import pytest

import layout_arena as A
import layout_cases as L
import vfgs_testlib as T
from test_gpu_kernel_keys import check_launch, program

pytestmark = pytest.mark.gpu

LDS = dict(L.K.fixture())


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from versatilefilmgrain_amd import hw
    h = hw.VfgsHip(device=0)
    yield h
    h.clear_chroma_mix()
    h.lib.vfgs_hip_reset_state()


class Memory:
    """the arena's bytes in one allocation of the case's kind, its base 256-byte aligned"""

    def __init__(self, hip, kind, buf):
        import torch
        self.hip, self.kind, self.pinned = hip, kind, None
        if kind == "device":
            self.t = torch.from_numpy(buf).cuda()
            self.base = self.t.data_ptr()
        else:
            if kind == "pinned":
                self.pinned = p = hip.host_alloc(buf.size + 256)
            else:
                self.keep = np.empty(buf.size + 256, np.uint8)
                p = self.keep.ctypes.data
            self.base = (p + 255) & ~255
            self.host = np.frombuffer((C.c_char * buf.size).from_address(self.base), dtype=np.uint8)
            self.host[...] = buf
        assert self.base % 256 == 0, "the arena's own base is 256-byte aligned: every residue of the layout is the plane's"

    def download(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy() if self.kind == "device" else self.host.copy()

    def free(self):
        if self.pinned:
            self.host = None
            self.hip.host_free(self.pinned)
            self.pinned = None


def invoke(hip, c, a, base, model):
    """the case's call, with pointers into the arena"""
    from gpu_util import stream_ptr
    stream = stream_ptr()
    n, e, w, h = c.nframes, c.entry, c.width, c.height
    side = "io" if c.dst is None else "src"
    ptrs = lambda sd, f, roles: tuple(base + a.plane(sd, f, r).off for r in roles)
    roles = lambda kind: ("Y", "UV") if kind in ("sp", "sp8") else ("Y", "U", "V")
    pitch = lambda sd, kind: [a.plane(sd, 0, r) for r in roles(kind)[:2]]
    (sy, sc) = pitch(side, c.src)
    st, cst, yp, cp = sy.pitch // sy.sz, sc.pitch // sc.sz, sy.pitch * sy.rows, sc.pitch * sc.rows
    src = [ptrs(side, f, roles(c.src)) for f in range(n)]
    dst = dst_st = dcst = dyp = dcp = None
    if c.dst is not None:
        (dy, dc) = pitch("dst", c.dst)
        dst_st, dcst, dyp, dcp = dy.pitch // dy.sz, dc.pitch // dc.sz, dy.pitch * dy.rows, dc.pitch * dc.rows
        dst = [ptrs("dst", f, roles(c.dst)) for f in range(n)]
    py, ph = c.part or (0, h)
    models = [model] * n
    seeds = c.seeds
    if e == "add_grain_stripe":
        hip.add_grain_stripe(*src[0], py, w, ph, st, cst)
    elif e == "add_grain_stripe_dev":
        hip.add_grain_stripe_dev(*src[0], py, w, ph, st, cst, stream)
    elif e == "add_grain_frame_dev":
        for f in range(n):
            hip.add_grain_frame_dev(*src[f], w, h, st, cst, stream)
    elif e == "add_grain_frame_part_dev":
        hip.add_grain_frame_part_dev(*src[0], w, h, py, ph, st, cst, stream)
    elif e == "add_grain_frames_dev":
        hip.add_grain_frames_dev(*src[0], w, h, st, cst, n, yp, cp, stream)
    elif e == "add_grain_frames_part_dev":
        hip.add_grain_frames_part_dev(*src[0], w, h, py, ph, st, cst, n, yp, cp, stream)
    elif e == "add_grain_copy_dev":
        hip.add_grain_copy_dev(*src[0], *dst[0], w, h, py, ph, st, cst, n, yp, cp, stream)
    elif e == "add_grain_copy8_dev":
        hip.add_grain_copy8_dev(*src[0], *dst[0], w, h, py, ph, st, cst, dst_st, dcst, n, yp, cp, dyp, dcp, stream)
    elif e == "add_grain_frame_list_dev":
        hip.add_grain_frame_list_dev(src, w, h, st, cst, stream)
    elif e == "add_grain_frame_list_part_dev":
        hip.add_grain_frame_list_part_dev(src, w, h, py, ph, st, cst, stream)
    elif e == "add_grain_frame_list_copy_dev":
        hip.add_grain_frame_list_copy_dev(src, dst, w, h, st, cst, stream)
    elif e == "add_grain_frame_list_copy8_dev":
        hip.add_grain_frame_list_copy8_dev(src, dst, w, h, st, cst, dst_st, dcst, stream)
    elif e == "add_grain_frame_list_seeded_dev":
        hip.add_grain_frame_list_seeded_dev(src, seeds, w, h, st, cst, stream)
    elif e == "add_grain_frame_list_seeded_part_dev":
        hip.add_grain_frame_list_seeded_part_dev(src, seeds, w, h, py, ph, st, cst, stream)
    elif e == "add_grain_frame_list_seeded_copy_dev":
        hip.add_grain_frame_list_seeded_copy_dev(src, dst, seeds, w, h, st, cst, stream)
    elif e == "add_grain_frame_list_seeded_copy8_dev":
        hip.add_grain_frame_list_seeded_copy8_dev(src, dst, seeds, w, h, st, cst, dst_st, dcst, stream)
    elif e == "add_grain_sp_frame_list_dev":
        hip.add_grain_sp_frame_list_dev(src, None, seeds, w, h, st, cst, c.shift, stream)
    elif e == "add_grain_sp_frame_list_copy8_dev":
        hip.add_grain_sp_frame_list_copy8_dev(src, dst, seeds, w, h, st, cst, dst_st, dcst, c.shift, stream)
    elif e == "add_grain_frame_list_to_sp_dev":
        hip.add_grain_frame_list_to_sp_dev(src, dst, seeds, w, h, st, cst, dst_st, dcst, c.shift, stream)
    elif e == "add_grain_frame_list_to_sp8_dev":
        hip.add_grain_frame_list_to_sp8_dev(src, dst, seeds, w, h, st, cst, dst_st, dcst, stream)
    elif e == "add_grain_frame_list_models_dev":
        hip.add_grain_frame_list_models_dev(src, None, models, seeds, w, h, st, cst, stream)
    elif e == "add_grain_sp_frame_list_models_dev":
        hip.add_grain_sp_frame_list_models_dev(src, None, models, seeds, w, h, st, cst, c.shift, stream)
    elif e == "add_grain_frame_list_models_copy8_dev":
        hip.add_grain_frame_list_models_copy8_dev(src, dst, models, seeds, w, h, st, cst, dst_st, dcst, stream)
    elif e == "add_grain_sp_frame_list_models_copy8_dev":
        hip.add_grain_sp_frame_list_models_copy8_dev(src, dst, models, seeds, w, h, st, cst, dst_st, dcst, c.shift, stream)
    elif e == "add_grain_frame_list_models_to_sp_dev":
        hip.add_grain_frame_list_models_to_sp_dev(src, dst, models, seeds, w, h, st, cst, dst_st, dcst, c.shift, stream)
    elif e == "add_grain_frame_list_models_to_sp8_dev":
        hip.add_grain_frame_list_models_to_sp8_dev(src, dst, models, seeds, w, h, st, cst, dst_st, dcst, stream)
    elif e == "add_grain_frames_host":
        hip.add_grain_frames_host(*[[s[k] for s in src] for k in range(3)], w, h, st, cst)
    elif e == "host_pipe":
        with hip.host_pipe(w, h, st, cst, dst_st or 0, dcst or 0, c.dst == "planar8") as pipe:
            tickets = [pipe.submit(src[f], None if dst is None else dst[f], model, seeds[f]) for f in range(n)]
            for t in tickets:
                pipe.wait(t)
    else:
        raise AssertionError(f"no call for {e}")
    return 1 if e == "add_grain_frame_dev" else n


FAULTED = []      # a HIP error is sticky: once the device has reported one, no later case of this module touches it


def run(hip, c):
    assert not FAULTED, f"not run: the device reported an error in an earlier case: {FAULTED[0]}"
    try:
        return _run(hip, c)
    except AssertionError:
        raise
    except Exception as e:
        import torch
        try:
            torch.cuda.synchronize()
        except Exception:
            FAULTED.append(f"{c.id}: {e}")
        raise


def _run(hip, c):
    from gpu_util import stream_ptr
    a = L.make_arena(c)
    want = L.expected(a, c)
    if c.mix:
        assert want.excluded / want.processed <= L.K.MIX_CAP, (want.excluded, want.processed)
    model = mem = None
    try:
        program(hip, L.records(c), c.mix)
        if c.models:
            model = hip.model_capture(stream_ptr())
        mem = Memory(hip, c.mem, a.buf)
        nframes = invoke(hip, c, a, mem.base, model)
        got = mem.download()
        A.compare(a, got, want.buf, want.compared, c.id)
        assert hip.seed_state() == want.regs, c.id
        return nframes
    finally:
        hip.clear_chroma_mix()
        if model is not None:
            hip.model_release(model)
        if mem is not None:
            mem.free()


@pytest.mark.parametrize("case", L.key_cases(), ids=lambda c: c.id)
def test_every_kernel_key_on_a_tight_layout(hip, case):
    nframes = run(hip, case)
    check_launch(hip, case.id, LDS[case.id], L.K.case_for(case.id), nframes)


@pytest.mark.parametrize("case", L.entry_cases(), ids=lambda c: c.id)
def test_every_entry_on_a_tight_layout(hip, case):
    run(hip, case)
