"""Helpers of the tests of vfgs_hip_add_grain_sp_frame_list_models_dev (TEST INFRASTRUCTURE): semi-planar frames with a model per picture.

The contract (include/vfgs_hip.h) is the loop of the planar models call with the one-frame semi-planar call in it:

    for f in list order:
        program the state models[f] was captured from
        if (seeds) vfgs_set_seed(seeds[f])
        vfgs_hip_add_grain_sp_frame_list_dev(&src[f], &dst[f], NULL, 1, ...)

so the ground truth is that loop on the oracle, composed from the two parents' helpers: a frame is grained as tests/semiplanar_util.py
grains it (the oracle on D(frame), interleaved again, shifted back, written over the whole blocks of the picture's rows) by an oracle that
holds the frame's model as tests/model_list_util.py arranges it -- a seed per picture: one oracle per model, reseeded per frame; one seed
sequence: ONE oracle into which the frame's model program is replayed without its seed records in front of the frame."""
import model_list_util as U
import semiplanar_util as SP


def expect_seeded(recs, pick, frames, seeds, shift):
    """-> (expected SPFrames, the four registers afterwards)"""
    oras = [U.oracle_programmed(r) for r in recs]
    want = []
    for sp, k, s in zip(frames, pick, seeds):
        want += SP.expected(oras[k], [sp], [s], shift)
    return want, oras[pick[-1]].seed_state()


def expect_unseeded(ora, recs, pick, frames, shift):
    """`ora`: a context whose registers are the library's in front of the call (model_list_util.oracle_programmed(recs[-1]) behind
    capture_all); it is left where the library is left, registers and -- of the last frame's model -- program"""
    import vfgs_testlib as T
    want = []
    for sp, k in zip(frames, pick):
        T.replay(ora, U.without_seed(recs[k]))
        want += SP.expected(ora, [sp], None, shift)
    return want, ora.seed_state()
