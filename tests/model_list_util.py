"""Helpers of the tests of models as device objects (TEST INFRASTRUCTURE): vfgs_hip_model_capture and
vfgs_hip_add_grain_frame_list_models_dev (include/vfgs_hip.h).

The contract of the call is a loop -- program the state models[f] was captured from; with seeds, vfgs_set_seed(seeds[f]); grain frame f --
and the ground truth is the oracle run as that loop:

* a seed per picture makes the frames independent: one OracleHW per model, reseeded per frame;
* one seed sequence: ONE oracle context into which the frame's model program is replayed WITHOUT its OP_SEED records before each frame
  (the setters do not touch the registers).  Slots a model's pattern LUT never selects do not reach the output, so leftovers of another
  model's program in the banks are harmless; what a program does not set at all would not be -- the SEI programs never set the range --
  so a model program here always begins with the power-on range (model_records).

A model is named by its trace in tests/golden/traces ("name"), at depth 12 by "name@depth12" (test_gpu_depth12.records12), or by the name of
a generated program (tests/model_programs.py)."""
import model_programs as MP
import vfgs_testlib as T

_names = None


def _generated():
    global _names
    if _names is None:
        _names = frozenset(MP.names())
    return _names


def model_records(name):
    if name in _generated():
        return MP.program(name)         # (a generated program sets everything, the range included)
    if name.endswith("@depth12"):
        import test_gpu_depth12 as D
        rec = D.records12(name[:-len("@depth12")])
    else:
        rec = T.load_trace(name)
    if not any(op == T.OP_LEGAL_RANGE for op, *_ in rec):
        rec = [(T.OP_LEGAL_RANGE, 0, 0, b"")] + list(rec)
    return rec


def without_seed(rec):
    return [r for r in rec if r[0] != T.OP_SEED]


def program(hip, rec):
    """the library programmed with `rec` from its power-on state (registers: the program's last seed)"""
    hip.lib.vfgs_hip_reset_state()
    T.replay(hip, rec)


def capture_all(hip, recs, stream=0):
    """program and capture in turn; the library stays programmed with recs[-1]"""
    models = []
    for rec in recs:
        program(hip, rec)
        models.append(hip.model_capture(stream))
    return models


def oracle_programmed(rec):
    ora = T.OracleHW()
    T.replay(ora, rec)
    return ora


def expect_seeded(recs, pick, frames, seeds):
    """-> (expected frames, the four registers afterwards)"""
    oras = [oracle_programmed(r) for r in recs]
    want = [f.copy() for f in frames]
    for w, k, s in zip(want, pick, seeds):
        oras[k].set_seed(s)
        oras[k].add_grain_frame(w)
    return want, oras[pick[-1]].seed_state()


def expect_unseeded(ora, recs, pick, frames):
    """`ora`: a context whose registers are the library's in front of the call (oracle_programmed(recs[-1]) behind capture_all);
    it is left where the library is left, registers and -- of the last frame's model -- program"""
    want = [f.copy() for f in frames]
    for w, k in zip(want, pick):
        T.replay(ora, without_seed(recs[k]))
        ora.add_grain_frame(w)
    return want, ora.seed_state()


def launches(hip):
    return (hip.last_launch_info() or {"launches": 0})["launches"]


def runs_of(forms, pick, limit=32):
    """lengths of the launches a list makes: runs of at most `limit` consecutive frames whose models share their form"""
    out = []
    for k in pick:
        if out and out[-1][0] == forms[k] and out[-1][1] < limit:
            out[-1][1] += 1
        else:
            out.append([forms[k], 1])
    return [n for _, n in out]
