"""ctypes mirror of include/vfgs_hip.h.

Same names and argument meaning as the reference hardware-layer interface
(/root/reference/src/vfgs_hw.h:51-62) plus the vfgs_hip_* extensions.  The library state is
a process-global singleton exactly like the reference's (vfgs_hw.c:49-68), so ``VfgsHip`` is
a namespace around that singleton, not an object with private state.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

from .build import LIB

_lib = None


class VfgsHipError(RuntimeError):
    pass


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so (same SONAME as /opt/rocm's) and opens it by path:
    if this library is loaded first it binds /opt/rocm's copy, a later `import torch` brings a second runtime into the process
    and whichever initialises second finds no device ("no ROCm-capable device is detected", seen when build() and smoke() ran in
    one process).  So where torch is installed but not imported yet, its copy is opened first (by the path torch itself will
    use) and libvfgs_hip.so's NEEDED entry resolves to it -- the arrangement every test and bench.py run has anyway (they import
    torch first).  Without torch (a C host) nothing happens and /opt/rocm's runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("VFGS_HIP_NO_TORCH_RUNTIME"):     # (opt out: a Python host that will never import torch)
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    rt = Path(spec.origin).parent / "lib" / "libamdhip64.so"
    if rt.exists():
        try:
            C.CDLL(str(rt), mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def hip_runtimes_mapped() -> list[str]:
    """Paths of every libamdhip64 mapped into this process (Linux): more than one means two HIP runtimes, and whichever
    initialises second finds no device."""
    out = []
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(None, 1)[-1] if "/" in line else ""
                if "libamdhip64" in path and path not in out:
                    out.append(path)
    except OSError:
        pass
    return out


def load(path: Path | None = None) -> C.CDLL:
    """dlopen libvfgs_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = Path(path or LIB)
    if not path.exists():
        raise VfgsHipError(f"{path} not built: run `python -m versatilefilmgrain_amd.build` "
                           "(needs hipcc); there is no CPU fallback")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(str(path))
    rts = hip_runtimes_mapped()
    if len(rts) > 1:
        import warnings
        warnings.warn(f"libvfgs_hip: {len(rts)} HIP runtimes are mapped into this process ({', '.join(rts)}): device calls of the one "
                      "that initialises second will fail.  Import torch before loading the library, or set VFGS_HIP_NO_TORCH_RUNTIME=1 "
                      "in a process that never imports torch.", RuntimeWarning, stacklevel=2)
    vp, u, i = C.c_void_p, C.c_uint, C.c_int
    lib.vfgs_set_luma_pattern.argtypes = [i, vp]
    lib.vfgs_set_chroma_pattern.argtypes = [i, vp]
    lib.vfgs_set_scale_lut.argtypes = [i, vp]
    lib.vfgs_set_pattern_lut.argtypes = [i, vp]
    lib.vfgs_set_seed.argtypes = [u]
    lib.vfgs_set_scale_shift.argtypes = [i]
    lib.vfgs_set_depth.argtypes = [i]
    lib.vfgs_set_legal_range.argtypes = [i]
    lib.vfgs_set_chroma_subsampling.argtypes = [i, i]
    lib.vfgs_add_grain_line.argtypes = [vp, vp, vp, i, i]
    lib.vfgs_add_grain_stripe.argtypes = [vp, vp, vp, u, u, u, u, u]
    lib.vfgs_hip_init.argtypes = [i]
    lib.vfgs_hip_init_devices.argtypes = [C.POINTER(i), i]
    lib.vfgs_hip_overlap_begin.argtypes = [vp]
    lib.vfgs_hip_get_stream_stats.argtypes = [C.POINTER(C.c_uint64)]
    lib.vfgs_hip_get_stream_stats.restype = None
    lib.vfgs_hip_get_stripe_stream_stats.argtypes = [C.POINTER(C.c_uint64)]
    lib.vfgs_hip_get_stripe_stream_stats.restype = None
    lib.vfgs_hip_lfsr_segments.argtypes = [u, C.c_uint64, C.c_uint64, u, u, C.POINTER(C.c_uint32)]
    lib.vfgs_hip_overlap_end.argtypes = [vp]
    lib.vfgs_hip_add_grain_stripe_dev.argtypes = [vp, vp, vp, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frame_dev.argtypes = [vp, vp, vp, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frame_part_dev.argtypes = [vp, vp, vp, u, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frames_dev.argtypes = [vp, vp, vp, u, u, u, u, u, C.c_uint64, C.c_uint64, vp]
    lib.vfgs_hip_add_grain_frames_part_dev.argtypes = [vp, vp, vp, u, u, u, u, u, u, u, C.c_uint64, C.c_uint64, vp]
    lib.vfgs_hip_add_grain_copy_dev.argtypes = [vp, vp, vp, vp, vp, vp, u, u, u, u, u, u, u, C.c_uint64, C.c_uint64, vp]
    lib.vfgs_hip_add_grain_copy8_dev.argtypes = [vp, vp, vp, vp, vp, vp, u, u, u, u, u, u, u, u, u,
                                                 C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, vp]
    fp = C.POINTER(FramePtrs)
    lib.vfgs_hip_add_grain_frame_list_dev.argtypes = [fp, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frame_list_part_dev.argtypes = [fp, u, u, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frame_list_copy_dev.argtypes = [fp, fp, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frame_list_copy8_dev.argtypes = [fp, fp, u, u, u, u, u, u, u, vp]
    sp = C.POINTER(C.c_uint32)
    lib.vfgs_hip_add_grain_frame_list_seeded_dev.argtypes = [fp, sp, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frame_list_seeded_part_dev.argtypes = [fp, sp, u, u, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frame_list_seeded_copy_dev.argtypes = [fp, fp, sp, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frame_list_seeded_copy8_dev.argtypes = [fp, fp, sp, u, u, u, u, u, u, u, vp]
    spf = C.POINTER(SpFrame)
    lib.vfgs_hip_add_grain_sp_frame_list_dev.argtypes = [spf, spf, sp, u, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_sp_frame_list_copy8_dev.argtypes = [spf, spf, sp, u, u, u, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frame_list_to_sp_dev.argtypes = [fp, spf, sp, u, u, u, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frame_list_to_sp8_dev.argtypes = [fp, spf, sp, u, u, u, u, u, u, u, vp]
    lib.vfgs_hip_model_capture.argtypes = [C.POINTER(vp), vp]
    lib.vfgs_hip_model_release.argtypes = [vp]
    lib.vfgs_hip_model_release.restype = None
    lib.vfgs_hip_model_info.argtypes = [vp, C.POINTER(i)]
    lib.vfgs_hip_model_image.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.vfgs_hip_get_model_build_stats.argtypes = [C.POINTER(C.c_uint64)]
    lib.vfgs_hip_get_model_build_stats.restype = None
    lib.vfgs_hip_models_from_afgs1.argtypes = [vp, u, C.POINTER(vp), vp]
    lib.vfgs_hip_models_from_sei.argtypes = [vp, u, C.POINTER(vp), vp]
    lib.vfgs_hip_models_from_afgs1_mix.argtypes = [vp, u, C.POINTER(vp), vp]
    lib.vfgs_hip_model_capture_mix.argtypes = [C.POINTER(vp), vp]
    lib.vfgs_hip_model_chroma_mix.argtypes = [vp, i, C.POINTER(i)]
    lib.vfgs_hip_add_grain_frame_list_models_dev.argtypes = [fp, fp, C.POINTER(vp), sp, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_sp_frame_list_models_dev.argtypes = [spf, spf, C.POINTER(vp), sp, u, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frame_list_models_copy8_dev.argtypes = [fp, fp, C.POINTER(vp), sp, u, u, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_sp_frame_list_models_copy8_dev.argtypes = [spf, spf, C.POINTER(vp), sp, u, u, u, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frame_list_models_to_sp_dev.argtypes = [fp, spf, C.POINTER(vp), sp, u, u, u, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_frame_list_models_to_sp8_dev.argtypes = [fp, spf, C.POINTER(vp), sp, u, u, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_sp_frame_list_to_planar_dev.argtypes = [spf, fp, sp, u, u, u, u, u, u, u, u, vp]
    lib.vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev.argtypes = [spf, fp, C.POINTER(vp), sp, u, u, u, u, u, u, u, u, vp]
    lib.vfgs_hip_seed_segments.argtypes = [sp, u, C.c_uint64, u, sp]
    lib.vfgs_hip_get_seeded_stream_stats.argtypes = [C.POINTER(C.c_uint64)]
    lib.vfgs_hip_get_seeded_stream_stats.restype = None
    lib.vfgs_hip_get_seed_state.argtypes = [vp]
    lib.vfgs_hip_get_luts.argtypes = [i, vp, vp]
    lib.vfgs_hip_get_params.argtypes = [vp]
    lib.vfgs_hip_get_params.restype = None
    lib.vfgs_hip_last_error_string.restype = C.c_char_p
    lib.vfgs_hip_timer_begin.argtypes = [vp]
    lib.vfgs_hip_timer_end.argtypes = [vp, C.POINTER(C.c_float)]
    lib.vfgs_hip_device_info.argtypes = [C.POINTER(i), C.POINTER(i), C.POINTER(i), C.c_char_p, i]
    lib.vfgs_hip_line_lookahead.argtypes = [i]
    lib.vfgs_hip_line_lookahead.restype = None
    lib.vfgs_hip_declare_frame.argtypes = [vp, vp, vp, u, u, u, u]
    lib.vfgs_hip_add_grain_frames_host.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), u, u, u, u, u]
    lib.vfgs_hip_host_pipe_open.argtypes = [C.POINTER(HostPipeDesc), C.POINTER(vp)]
    lib.vfgs_hip_host_pipe_submit.argtypes = [vp, fp, fp, vp, sp, C.POINTER(C.c_uint64)]
    lib.vfgs_hip_host_pipe_wait.argtypes = [vp, C.c_uint64]
    lib.vfgs_hip_host_pipe_close.argtypes = [vp]
    lib.vfgs_hip_host_alloc.argtypes = [C.c_uint64]
    lib.vfgs_hip_host_alloc.restype = vp
    lib.vfgs_hip_host_free.argtypes = [vp]
    lib.vfgs_hip_host_free.restype = None
    lib.vfgs_hip_last_launch_info.argtypes = [C.POINTER(LaunchInfo)]
    lib.vfgs_hip_set_chroma_mix.argtypes = [i, i, i, i]
    lib.vfgs_hip_clear_chroma_mix.argtypes = []
    lib.vfgs_hip_clear_chroma_mix.restype = None
    lib.vfgs_hip_get_chroma_mix.argtypes = [i, C.POINTER(i)]
    lib.vfgs_hip_supports_depth.argtypes = [i]
    # a library built by a developer tool with tuning / ablation knobs may compute something else by design: only on request
    if lib.vfgs_hip_dev_build() and not os.environ.get("VFGS_ALLOW_DEV_BUILD"):
        raise VfgsHipError(f"{path} is a developer build (tuning / ablation knobs); set VFGS_ALLOW_DEV_BUILD=1 to load it anyway")
    _lib = lib
    return lib


class LaunchInfo(C.Structure):
    """include/vfgs_hip.h: vfgs_hip_launch_info."""
    _fields_ = [("depth", C.c_int), ("csubx", C.c_int), ("csuby", C.c_int), ("out8", C.c_int), ("one_y", C.c_int), ("one_c", C.c_int),
                ("in_place", C.c_int), ("nframes", C.c_int), ("workgroups_per_frame", C.c_int), ("frames_per_front", C.c_int),
                ("rows_per_wave", C.c_int * 2), ("positions_per_row", C.c_int * 2), ("parts_per_row", C.c_int), ("persistent_luma_workgroups", C.c_int),
                ("waves_per_workgroup", C.c_int), ("lds_bytes_per_workgroup", C.c_int), ("launches", C.c_ulonglong), ("kernel", C.c_char * 96), ("listed", C.c_int), ("internal", C.c_int)]


class FramePtrs(C.Structure):
    """include/vfgs_hip.h: vfgs_hip_frame_ptrs (device pointers to line 0 of one frame's planes)."""
    _fields_ = [("Y", C.c_void_p), ("U", C.c_void_p), ("V", C.c_void_p)]


class HostPipeDesc(C.Structure):
    """include/vfgs_hip.h: vfgs_hip_host_pipe_desc."""
    _fields_ = [("width", C.c_uint), ("height", C.c_uint), ("stride", C.c_uint), ("cstride", C.c_uint), ("dst_stride", C.c_uint),
                ("dst_cstride", C.c_uint), ("dst8", C.c_int), ("slots", C.c_uint)]


class SpFrame(C.Structure):
    """include/vfgs_hip.h: vfgs_hip_sp_frame (device pointers to line 0 of a semi-planar frame's luma plane and its plane of Cb/Cr pairs)."""
    _fields_ = [("Y", C.c_void_p), ("UV", C.c_void_p)]


EXPORTS = [
    # drop-in, vfgs_hw.h:51-62
    "vfgs_set_luma_pattern", "vfgs_set_chroma_pattern", "vfgs_set_scale_lut", "vfgs_set_pattern_lut",
    "vfgs_set_seed", "vfgs_set_scale_shift", "vfgs_set_depth", "vfgs_set_legal_range",
    "vfgs_set_chroma_subsampling", "vfgs_add_grain_line",
    # extensions
    "vfgs_add_grain_stripe", "vfgs_hip_init", "vfgs_hip_shutdown", "vfgs_hip_reset_state",
    "vfgs_hip_add_grain_stripe_dev", "vfgs_hip_add_grain_frame_dev", "vfgs_hip_add_grain_frame_part_dev",
    "vfgs_hip_add_grain_frames_dev", "vfgs_hip_add_grain_frames_part_dev", "vfgs_hip_add_grain_copy_dev",
    "vfgs_hip_add_grain_copy8_dev", "vfgs_hip_add_grain_frame_list_dev", "vfgs_hip_add_grain_frame_list_part_dev", "vfgs_hip_add_grain_frame_list_copy_dev",
    "vfgs_hip_add_grain_frame_list_copy8_dev", "vfgs_hip_get_seed_state", "vfgs_hip_get_luts", "vfgs_hip_get_params", "vfgs_hip_last_error",
    "vfgs_hip_last_error_string", "vfgs_hip_timer_begin", "vfgs_hip_timer_end", "vfgs_hip_device_info",
    "vfgs_hip_dev_build", "vfgs_hip_init_devices", "vfgs_hip_overlap_begin", "vfgs_hip_overlap_end", "vfgs_hip_get_stream_stats", "vfgs_hip_line_lookahead", "vfgs_hip_declare_frame",
    "vfgs_hip_get_stripe_stream_stats", "vfgs_hip_lfsr_segments",
    "vfgs_hip_add_grain_frame_list_seeded_dev", "vfgs_hip_add_grain_frame_list_seeded_part_dev", "vfgs_hip_add_grain_frame_list_seeded_copy_dev",
    "vfgs_hip_add_grain_frame_list_seeded_copy8_dev", "vfgs_hip_add_grain_sp_frame_list_dev", "vfgs_hip_add_grain_sp_frame_list_copy8_dev",
    "vfgs_hip_add_grain_frame_list_to_sp_dev", "vfgs_hip_add_grain_frame_list_to_sp8_dev", "vfgs_hip_seed_segments", "vfgs_hip_get_seeded_stream_stats",
    "vfgs_hip_add_grain_frames_host", "vfgs_hip_host_alloc", "vfgs_hip_host_free", "vfgs_hip_last_launch_info",
    "vfgs_hip_set_chroma_mix", "vfgs_hip_clear_chroma_mix", "vfgs_hip_get_chroma_mix", "vfgs_hip_supports_depth",
    "vfgs_hip_model_capture", "vfgs_hip_model_capture_mix", "vfgs_hip_model_chroma_mix", "vfgs_hip_model_release", "vfgs_hip_model_info", "vfgs_hip_add_grain_frame_list_models_dev",
    "vfgs_hip_add_grain_sp_frame_list_models_dev", "vfgs_hip_model_image", "vfgs_hip_get_model_build_stats",
    "vfgs_hip_add_grain_frame_list_models_copy8_dev", "vfgs_hip_add_grain_sp_frame_list_models_copy8_dev",
    "vfgs_hip_add_grain_frame_list_models_to_sp_dev", "vfgs_hip_add_grain_frame_list_models_to_sp8_dev",
    "vfgs_hip_add_grain_sp_frame_list_to_planar_dev", "vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev",
    "vfgs_hip_host_pipe_open", "vfgs_hip_host_pipe_submit", "vfgs_hip_host_pipe_wait", "vfgs_hip_host_pipe_close",
]


def _b(data):
    return (C.c_char * len(data)).from_buffer_copy(bytes(data))


class VfgsHip:
    """Namespace over the library singleton (same method names as the test-side wrappers)."""

    def __init__(self, device: int | None = None, reset: bool = True):
        self.lib = load()
        if device is not None:
            self._ck(self.lib.vfgs_hip_init(device))
        if reset:
            self.lib.vfgs_hip_reset_state()

    def _ck(self, rc):
        if rc:
            raise VfgsHipError(f"libvfgs_hip error {rc}: {self.lib.vfgs_hip_last_error_string().decode()}")

    # ---- drop-in setters
    def set_luma_pattern(self, i, P):       self.lib.vfgs_set_luma_pattern(i, _b(P))
    def set_chroma_pattern(self, i, P):     self.lib.vfgs_set_chroma_pattern(i, _b(P))
    def set_scale_lut(self, c, lut):        self.lib.vfgs_set_scale_lut(c, _b(lut))
    def set_pattern_lut(self, c, lut):      self.lib.vfgs_set_pattern_lut(c, _b(lut))
    def set_seed(self, s):                  self.lib.vfgs_set_seed(s & 0xFFFFFFFF)
    def set_scale_shift(self, s):           self.lib.vfgs_set_scale_shift(s)
    def set_depth(self, d):                 self.lib.vfgs_set_depth(d)
    def supports_depth(self, d):            return bool(self.lib.vfgs_hip_supports_depth(d))     # (vfgs_set_depth aborts on any other)
    def set_legal_range(self, l):           self.lib.vfgs_set_legal_range(l)
    def set_chroma_subsampling(self, x, y): self.lib.vfgs_set_chroma_subsampling(x, y)

    # ---- host-memory processing (pointers are plain integers / ctypes addresses)
    def add_grain_line(self, Y, U, V, y, width):
        self.lib.vfgs_add_grain_line(Y, U, V, y, width)

    def add_grain_stripe(self, Y, U, V, y, width, height, stride, cstride):
        self.lib.vfgs_add_grain_stripe(Y, U, V, y, width, height, stride, cstride)

    # ---- device-resident processing
    def add_grain_stripe_dev(self, dY, dU, dV, y, width, height, stride, cstride, stream=0):
        self._ck(self.lib.vfgs_hip_add_grain_stripe_dev(dY, dU, dV, y, width, height, stride, cstride, stream))

    def add_grain_frame_dev(self, dY, dU, dV, width, height, stride, cstride, stream=0):
        self._ck(self.lib.vfgs_hip_add_grain_frame_dev(dY, dU, dV, width, height, stride, cstride, stream))

    def add_grain_frame_part_dev(self, dY, dU, dV, width, frame_height, part_y, part_height, stride, cstride, stream=0):
        self._ck(self.lib.vfgs_hip_add_grain_frame_part_dev(dY, dU, dV, width, frame_height, part_y, part_height,
                                                            stride, cstride, stream))

    def add_grain_frames_dev(self, dY, dU, dV, width, height, stride, cstride, nframes, ypitch, cpitch, stream=0):
        self._ck(self.lib.vfgs_hip_add_grain_frames_dev(dY, dU, dV, width, height, stride, cstride, nframes,
                                                        ypitch, cpitch, stream))

    def add_grain_frames_part_dev(self, dY, dU, dV, width, frame_height, part_y, part_height, stride, cstride,
                                  nframes, ypitch, cpitch, stream=0):
        self._ck(self.lib.vfgs_hip_add_grain_frames_part_dev(dY, dU, dV, width, frame_height, part_y, part_height,
                                                             stride, cstride, nframes, ypitch, cpitch, stream))

    def add_grain_copy_dev(self, sY, sU, sV, dY, dU, dV, width, frame_height, part_y, part_height, stride, cstride,
                           nframes, ypitch, cpitch, stream=0):
        self._ck(self.lib.vfgs_hip_add_grain_copy_dev(sY, sU, sV, dY, dU, dV, width, frame_height, part_y, part_height,
                                                      stride, cstride, nframes, ypitch, cpitch, stream))

    def add_grain_copy8_dev(self, sY, sU, sV, dY, dU, dV, width, frame_height, part_y, part_height, stride, cstride,
                            dstride, dcstride, nframes, ypitch, cpitch, dypitch, dcpitch, stream=0):
        self._ck(self.lib.vfgs_hip_add_grain_copy8_dev(sY, sU, sV, dY, dU, dV, width, frame_height, part_y, part_height,
                                                       stride, cstride, dstride, dcstride, nframes, ypitch, cpitch,
                                                       dypitch, dcpitch, stream))

    @staticmethod
    def frame_list(frames):
        """frames: sequence of (Y, U, V) device addresses -> ctypes array of vfgs_hip_frame_ptrs (build it once for a pool of
        frames that is handed over again and again; the list calls take either form)."""
        if isinstance(frames, C.Array):
            return frames
        arr = (FramePtrs * len(frames))()
        for k, (y, u_, v) in enumerate(frames):
            arr[k].Y, arr[k].U, arr[k].V = y, u_, v
        return arr

    def add_grain_frame_list_dev(self, frames, width, height, stride, cstride, stream=0):
        """Frames anywhere in device memory, one launch per 32 of them (include/vfgs_hip.h)."""
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_dev(self.frame_list(frames), len(frames), width, height, stride, cstride, stream))

    def add_grain_frame_list_part_dev(self, frames, width, frame_height, part_y, part_height, stride, cstride, stream=0):
        """Lines [part_y, part_y + part_height) of every listed frame; the pointers address line part_y; seeds advance as for whole frames."""
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_part_dev(self.frame_list(frames), len(frames), width, frame_height, part_y, part_height,
                                                                 stride, cstride, stream))

    def add_grain_frame_list_copy_dev(self, src, dst, width, height, stride, cstride, stream=0):
        assert len(src) == len(dst)
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_copy_dev(self.frame_list(src), self.frame_list(dst), len(src), width, height,
                                                                 stride, cstride, stream))

    def add_grain_frame_list_copy8_dev(self, src, dst, width, height, stride, cstride, dstride, dcstride, stream=0):
        assert len(src) == len(dst)
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_copy8_dev(self.frame_list(src), self.frame_list(dst), len(src), width, height,
                                                                  stride, cstride, dstride, dcstride, stream))

    @staticmethod
    def seed_list(seeds):
        """seeds: sequence of integers (what vfgs_set_seed would get, one per frame) -> ctypes uint32 array; None stays NULL."""
        if seeds is None or isinstance(seeds, C.Array):
            return seeds
        return (C.c_uint32 * len(seeds))(*[int(s) & 0xFFFFFFFF for s in seeds])

    def add_grain_frame_list_seeded_dev(self, frames, seeds, width, height, stride, cstride, stream=0):
        """The list call with a seed per picture: vfgs_set_seed(seeds[f]) + frame f, for every f, in one launch per 32 frames."""
        assert seeds is None or len(seeds) == len(frames)
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_seeded_dev(self.frame_list(frames), self.seed_list(seeds), len(frames), width, height,
                                                                   stride, cstride, stream))

    def add_grain_frame_list_seeded_part_dev(self, frames, seeds, width, frame_height, part_y, part_height, stride, cstride, stream=0):
        assert seeds is None or len(seeds) == len(frames)
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_seeded_part_dev(self.frame_list(frames), self.seed_list(seeds), len(frames), width, frame_height,
                                                                        part_y, part_height, stride, cstride, stream))

    def add_grain_frame_list_seeded_copy_dev(self, src, dst, seeds, width, height, stride, cstride, stream=0):
        assert len(src) == len(dst) and (seeds is None or len(seeds) == len(src))
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_seeded_copy_dev(self.frame_list(src), self.frame_list(dst), self.seed_list(seeds), len(src),
                                                                        width, height, stride, cstride, stream))

    def add_grain_frame_list_seeded_copy8_dev(self, src, dst, seeds, width, height, stride, cstride, dstride, dcstride, stream=0):
        assert len(src) == len(dst) and (seeds is None or len(seeds) == len(src))
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_seeded_copy8_dev(self.frame_list(src), self.frame_list(dst), self.seed_list(seeds), len(src),
                                                                         width, height, stride, cstride, dstride, dcstride, stream))

    @staticmethod
    def sp_frame_list(frames):
        """frames: sequence of (Y, UV) device addresses -> ctypes array of vfgs_hip_sp_frame (like frame_list)."""
        if isinstance(frames, C.Array):
            return frames
        arr = (SpFrame * len(frames))()
        for k, (y, uv) in enumerate(frames):
            arr[k].Y, arr[k].UV = y, uv
        return arr

    def add_grain_sp_frame_list_dev(self, src, dst, seeds, width, height, stride, uv_stride, sample_shift, stream=0):
        """Semi-planar frames (NV12 / NV16 / P010 / P210 / P012): a luma plane and one plane of Cb/Cr pairs each; dst is src (or None): in
        place; seeds None: one seed sequence, else a seed per picture; sample_shift 0 or 16 - depth (include/vfgs_hip.h).  An active chroma mix
        (set_chroma_mix, or the firmware's AFGS1 programming) is honoured for one-pattern models at depth 8 and 10: the result is the planar
        copy list's on the de-interleaved picture under the same mix; where a destination Y shares bytes with a source Y the call is two
        launches (UV rows first).  A general-form model or depth 12 under a mix: VfgsHipError 40, nothing changed."""
        s = self.sp_frame_list(src)
        d = s if (dst is None or dst is src) else self.sp_frame_list(dst)
        assert len(s) == len(d) and (seeds is None or len(seeds) == len(s))
        self._ck(self.lib.vfgs_hip_add_grain_sp_frame_list_dev(s, d, self.seed_list(seeds), len(s), width, height, stride, uv_stride,
                                                               sample_shift, stream))

    def add_grain_sp_frame_list_copy8_dev(self, src, dst, seeds, width, height, stride, uv_stride, dst_stride, dst_uv_stride, sample_shift, stream=0):
        """Semi-planar frames with the narrowed 8-bit destination (P010 / P210 / P012 -> NV12 / NV16): src as in add_grain_sp_frame_list_dev at
        depth 10 or 12 (strides in 16-bit containers), dst frames of bytes (strides in bytes), never in place; seeds None: one seed sequence.
        The bytes are the planar copy8 list's on the de-interleaved picture, interleaved again.  Depth 8: VfgsHipError 16; an active chroma
        mix: 40; a destination that shares bytes with any source plane: 18 (include/vfgs_hip.h)."""
        s, d = self.sp_frame_list(src), self.sp_frame_list(dst)
        assert len(s) == len(d) and (seeds is None or len(seeds) == len(s))
        self._ck(self.lib.vfgs_hip_add_grain_sp_frame_list_copy8_dev(s, d, self.seed_list(seeds), len(s), width, height, stride, uv_stride,
                                                                     dst_stride, dst_uv_stride, sample_shift, stream))

    def add_grain_frame_list_to_sp_dev(self, src, dst, seeds, width, height, stride, cstride, dst_stride, dst_uv_stride, sample_shift, stream=0):
        """Planar frames in, semi-planar surfaces out (yuv420p10le -> P010, yuv420p -> NV12 ...): src a list of (Y, U, V) addresses of planar,
        low-aligned pictures (strides in samples), dst a list of (Y, UV) addresses (strides in containers), never in place; seeds None: one
        seed sequence, else a seed per picture; sample_shift 0 or 16 - depth.  Every container is the planar copy list's sample
        << sample_shift, Cb and Cr interleaved.  An active chroma mix: VfgsHipError 40; a destination that shares bytes with any source
        plane: 18 (include/vfgs_hip.h)."""
        s, d = self.frame_list(src), self.sp_frame_list(dst)
        assert len(s) == len(d) and (seeds is None or len(seeds) == len(s))
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_to_sp_dev(s, d, self.seed_list(seeds), len(s), width, height, stride, cstride,
                                                                  dst_stride, dst_uv_stride, sample_shift, stream))

    def add_grain_frame_list_to_sp8_dev(self, src, dst, seeds, width, height, stride, cstride, dst_stride, dst_uv_stride, stream=0):
        """... with the narrowed 8-bit destination (planar 10 / 12 bit -> NV12 / NV16): dst frames of bytes, strides in bytes; the bytes are
        the planar copy8 list's, Cb and Cr interleaved.  Depth 8: VfgsHipError 16 (include/vfgs_hip.h)."""
        s, d = self.frame_list(src), self.sp_frame_list(dst)
        assert len(s) == len(d) and (seeds is None or len(seeds) == len(s))
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_to_sp8_dev(s, d, self.seed_list(seeds), len(s), width, height, stride, cstride,
                                                                   dst_stride, dst_uv_stride, stream))

    # ---- models as device objects (include/vfgs_hip.h)
    def model_capture(self, stream=0):
        """Snapshot of what is programmed now -- patterns (device-generated ones included), LUTs, scale shift, range, at the programmed depth
        and chroma format -- as a device-resident model; returns its handle (an integer).  Asynchronous on `stream`; nothing else changes."""
        m = C.c_void_p()
        self._ck(self.lib.vfgs_hip_model_capture(C.byref(m), stream))
        return m.value

    def model_release(self, m):
        """Release a model (None: no-op); allowed as soon as the call that used it has returned."""
        self.lib.vfgs_hip_model_release(m)

    def model_info(self, m):
        out = (C.c_int * 8)()
        self._ck(self.lib.vfgs_hip_model_info(m, out))
        return dict(zip(("depth", "csubx", "csuby", "one_y", "one_c", "scale_shift", "legal_range", "device_bytes"), out))

    def models_from_afgs1(self, cfgs, stream=0):
        """Models straight from AFGS1 parameter sets (fw.FgsAfgs1 objects), one kernel launch per 32 of them, at the programmed depth and chroma
        format: handles like model_capture's, each what `fw.afgs1_chroma_mix(False); fw.init_afgs1(cfg); model_capture()` would give, with
        the programmed state untouched.  The pictures' seeds are fw.afgs1_seed(cfg), for the list call.  VfgsHipError 42: a parameter set
        vfgs_init_afgs1 would abort on (the message names its index), 9: grain_scaling out of range; nothing is built then."""
        from . import fw
        cfgs = list(cfgs)
        if not cfgs:
            return []
        arr = (fw.FgsAfgs1 * len(cfgs))(*cfgs)
        out = (C.c_void_p * len(cfgs))()
        self._ck(self.lib.vfgs_hip_models_from_afgs1(arr, len(cfgs), out, stream))
        return list(out)

    def models_from_afgs1_mix(self, cfgs, stream=0):
        """models_from_afgs1 whose models also CARRY the chroma mix of their parameter set -- what `fw.afgs1_chroma_mix(True);
        fw.init_afgs1(cfg); model_capture_mix()` would give, whatever the switch says, with the programmed state (mix and switch included)
        untouched.  The two list calls with a model per picture honour the mix frame by frame.  VfgsHipError as models_from_afgs1, and 42: a mix
        field set_chroma_mix would refuse; 38: depth 12, or (8 bit) a scaling function that would need the general form."""
        from . import fw
        cfgs = list(cfgs)
        if not cfgs:
            return []
        arr = (fw.FgsAfgs1 * len(cfgs))(*cfgs)
        out = (C.c_void_p * len(cfgs))()
        self._ck(self.lib.vfgs_hip_models_from_afgs1_mix(arr, len(cfgs), out, stream))
        return list(out)

    def model_capture_mix(self, stream=0):
        """model_capture plus the chroma mix that is active now: the model carries it (none active: model_capture's result).  VfgsHipError
        38 where a processing call would refuse the programmed state under that mix: depth 12, a general-form model."""
        m = C.c_void_p()
        self._ck(self.lib.vfgs_hip_model_capture_mix(C.byref(m), stream))
        return m.value

    def model_chroma_mix(self, m, c):
        """(luma_mult, chroma_mult, offset, active) of component c (1 = Cb, 2 = Cr) as model m carries them; all zero: no mix."""
        out = (C.c_int * 4)()
        self._ck(self.lib.vfgs_hip_model_chroma_mix(m, c, out))
        return tuple(out)

    def models_from_sei(self, cfgs, stream=0):
        """Models straight from FGC SEI messages (fw.FgsSei objects), one kernel launch per 32 of them, at the programmed depth, chroma format
        and legal range: handles like model_capture's, each what `reset_state(); <depth, format, range>; fw.init_sei(cfg); model_capture()`
        would give, byte for byte in every form, with the programmed state untouched.  A message carries no seed: the pictures' seeds are the
        caller's, for the list call.  VfgsHipError 42: a message vfgs_init_sei would abort on or read past (the message names its index),
        9: log2_scale_factor out of range; nothing is built then."""
        from . import fw
        cfgs = list(cfgs)
        if not cfgs:
            return []
        arr = (fw.FgsSei * len(cfgs))(*cfgs)
        out = (C.c_void_p * len(cfgs))()
        self._ck(self.lib.vfgs_hip_models_from_sei(arr, len(cfgs), out, stream))
        return list(out)

    def model_image(self, m):
        """The model's 32-byte record and table image as the device holds them (bytes).  Synchronises; for tests and debugging."""
        need = C.c_size_t(0)
        rc = self.lib.vfgs_hip_model_image(m, None, 0, C.byref(need))
        if rc != 6:
            self._ck(rc)
        buf = C.create_string_buffer(need.value)
        self._ck(self.lib.vfgs_hip_model_image(m, buf, need.value, C.byref(need)))
        return buf.raw

    def model_build_stats(self):
        out = (C.c_uint64 * 8)()
        self.lib.vfgs_hip_get_model_build_stats(out)
        return dict(zip(("calls", "models", "launches", "copies", "allocations", "frees", "models_per_launch"), out))

    def add_grain_frame_list_models_dev(self, src, dst, models, seeds, width, height, stride, cstride, stream=0):
        """The list call with a model per picture: frame f is grained as if models[f]'s state were programmed (and, with seeds,
        vfgs_set_seed(seeds[f]) called) in front of it; one launch per run of at most 32 frames whose models share the form of their images.
        dst is src (or None): in place.  The programmed state is unchanged.  VfgsHipError 41: a null / released model, a model of another
        depth or chroma format, width > 8192, an active chroma mix."""
        s = self.frame_list(src)
        d = s if (dst is None or dst is src) else self.frame_list(dst)
        assert len(s) == len(d) == len(models) and (seeds is None or len(seeds) == len(s))
        arr = models if isinstance(models, C.Array) else (C.c_void_p * len(models))(*models)
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_models_dev(s, d, arr, self.seed_list(seeds), len(s), width, height, stride, cstride, stream))

    def add_grain_sp_frame_list_models_dev(self, src, dst, models, seeds, width, height, stride, uv_stride, sample_shift, stream=0):
        """Semi-planar frames with a model per picture: src / dst / seeds / geometry / sample_shift as in add_grain_sp_frame_list_dev (dst is
        src, or None: in place), models as in add_grain_frame_list_models_dev.  Frame f is grained as if models[f]'s state were programmed
        (and, with seeds, vfgs_set_seed(seeds[f]) called) in front of a one-frame add_grain_sp_frame_list_dev without a mix; one launch per
        run of at most 32 frames whose models share the form of their images.  The programmed state is unchanged.  VfgsHipError 40: csubx
        != 2, a bad sample_shift, width > 8192; 41: a null / released model, a model of another depth or chroma format, an active chroma mix."""
        s = self.sp_frame_list(src)
        d = s if (dst is None or dst is src) else self.sp_frame_list(dst)
        assert len(s) == len(d) == len(models) and (seeds is None or len(seeds) == len(s))
        arr = models if isinstance(models, C.Array) else (C.c_void_p * len(models))(*models)
        self._ck(self.lib.vfgs_hip_add_grain_sp_frame_list_models_dev(s, d, arr, self.seed_list(seeds), len(s), width, height, stride, uv_stride,
                                                                      sample_shift, stream))

    def add_grain_frame_list_models_copy8_dev(self, src, dst, models, seeds, width, height, stride, cstride, dstride, dcstride, stream=0):
        """A model per picture with the narrowed 8-bit destination: src as in add_grain_frame_list_copy8_dev (planar, depth 10 or 12), dst
        planar frames of bytes (strides in bytes), models and seeds as in add_grain_frame_list_models_dev.  Frame f gets the bytes of a
        one-frame add_grain_frame_list_copy8_dev with models[f]'s state programmed (and, with seeds, vfgs_set_seed(seeds[f]) called); one
        launch per run of at most 32 frames whose models share the form of their images; the programmed state is unchanged.  VfgsHipError
        16: depth 8; 41: a null / released model, a model of another depth or chroma format, width > 8192, an active chroma mix, a model
        that carries a mix (include/vfgs_hip.h)."""
        s, d = self.frame_list(src), self.frame_list(dst)
        assert len(s) == len(d) == len(models) and (seeds is None or len(seeds) == len(s))
        arr = models if isinstance(models, C.Array) else (C.c_void_p * len(models))(*models)
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_models_copy8_dev(s, d, arr, self.seed_list(seeds), len(s), width, height, stride, cstride,
                                                                         dstride, dcstride, stream))

    def add_grain_sp_frame_list_models_copy8_dev(self, src, dst, models, seeds, width, height, stride, uv_stride, dst_stride, dst_uv_stride,
                                                 sample_shift, stream=0):
        """... on semi-planar surfaces (P010 / P210 / P012 -> NV12 / NV16 with a model per picture): src / dst / strides / sample_shift as in
        add_grain_sp_frame_list_copy8_dev (never in place), models and seeds as above.  VfgsHipError 16: depth 8; 40: csubx != 2, a bad
        sample_shift, width > 8192; 41: as above; 18: a destination that shares bytes with any source plane (include/vfgs_hip.h)."""
        s, d = self.sp_frame_list(src), self.sp_frame_list(dst)
        assert len(s) == len(d) == len(models) and (seeds is None or len(seeds) == len(s))
        arr = models if isinstance(models, C.Array) else (C.c_void_p * len(models))(*models)
        self._ck(self.lib.vfgs_hip_add_grain_sp_frame_list_models_copy8_dev(s, d, arr, self.seed_list(seeds), len(s), width, height, stride, uv_stride,
                                                                            dst_stride, dst_uv_stride, sample_shift, stream))

    def add_grain_frame_list_models_to_sp_dev(self, src, dst, models, seeds, width, height, stride, cstride, dst_stride, dst_uv_stride,
                                              sample_shift, stream=0):
        """Planar frames in, semi-planar surfaces out, a model per picture (what a software decoder hands out, each picture with its own film
        grain parameters, onto P010 / NV12 ...): src / dst / strides / sample_shift as in add_grain_frame_list_to_sp_dev (never in place),
        models and seeds as in add_grain_frame_list_models_dev.  Frame f gets the containers of a one-frame add_grain_frame_list_to_sp_dev
        with models[f]'s state programmed (and, with seeds, vfgs_set_seed(seeds[f]) called); one launch per run of at most 32 frames whose
        models share the form of their images; the programmed state is unchanged.  VfgsHipError 40: csubx != 2, a bad sample_shift, width
        > 8192; 41: a null / released model, a model of another depth or chroma format, an active chroma mix, a model that carries a mix;
        18: a destination that shares bytes with any source plane (include/vfgs_hip.h)."""
        s, d = self.frame_list(src), self.sp_frame_list(dst)
        assert len(s) == len(d) == len(models) and (seeds is None or len(seeds) == len(s))
        arr = models if isinstance(models, C.Array) else (C.c_void_p * len(models))(*models)
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_models_to_sp_dev(s, d, arr, self.seed_list(seeds), len(s), width, height, stride, cstride,
                                                                         dst_stride, dst_uv_stride, sample_shift, stream))

    def add_grain_frame_list_models_to_sp8_dev(self, src, dst, models, seeds, width, height, stride, cstride, dst_stride, dst_uv_stride, stream=0):
        """... with the narrowed 8-bit destination (planar 10 / 12 bit -> NV12 / NV16 with a model per picture): dst frames of bytes, strides in
        bytes, as in add_grain_frame_list_to_sp8_dev; models and seeds as above.  VfgsHipError 16: depth 8; otherwise as above
        (include/vfgs_hip.h)."""
        s, d = self.frame_list(src), self.sp_frame_list(dst)
        assert len(s) == len(d) == len(models) and (seeds is None or len(seeds) == len(s))
        arr = models if isinstance(models, C.Array) else (C.c_void_p * len(models))(*models)
        self._ck(self.lib.vfgs_hip_add_grain_frame_list_models_to_sp8_dev(s, d, arr, self.seed_list(seeds), len(s), width, height, stride, cstride,
                                                                          dst_stride, dst_uv_stride, stream))

    def add_grain_sp_frame_list_to_planar_dev(self, src, dst, seeds, width, height, stride, uv_stride, dst_stride, dst_cstride, sample_shift, stream=0):
        """Semi-planar surfaces in, planar frames out (P010 -> yuv420p10le, NV12 -> yuv420p ...): src a list of (Y, UV) addresses as in
        add_grain_sp_frame_list_dev (strides in containers, sample_shift 0 or 16 - depth: the SOURCE's), dst a list of (Y, U, V) addresses of
        planar, low-aligned pictures (strides in samples), never in place; seeds None: one seed sequence, else a seed per picture.  Every
        sample is the out-of-place semi-planar call's container >> sample_shift, Cb and Cr de-interleaved.  An active chroma mix:
        VfgsHipError 40; a destination that shares bytes with another destination plane or any source plane: 18 (include/vfgs_hip.h)."""
        s, d = self.sp_frame_list(src), self.frame_list(dst)
        assert len(s) == len(d) and (seeds is None or len(seeds) == len(s))
        self._ck(self.lib.vfgs_hip_add_grain_sp_frame_list_to_planar_dev(s, d, self.seed_list(seeds), len(s), width, height, stride, uv_stride,
                                                                         dst_stride, dst_cstride, sample_shift, stream))

    def add_grain_sp_frame_list_models_to_planar_dev(self, src, dst, models, seeds, width, height, stride, uv_stride, dst_stride, dst_cstride,
                                                     sample_shift, stream=0):
        """... with a model per picture: src / dst / strides / sample_shift as in add_grain_sp_frame_list_to_planar_dev, models and seeds as in
        add_grain_sp_frame_list_models_dev.  Frame f gets the samples of a one-frame add_grain_sp_frame_list_to_planar_dev with models[f]'s
        state programmed (and, with seeds, vfgs_set_seed(seeds[f]) called); one launch per run of at most 32 frames whose models share the
        form of their images; the programmed state is unchanged.  VfgsHipError 40: csubx != 2, a bad sample_shift, width > 8192; 41: a null /
        released model, a model of another depth or chroma format, an active chroma mix, a model that carries a mix (include/vfgs_hip.h)."""
        s, d = self.sp_frame_list(src), self.frame_list(dst)
        assert len(s) == len(d) == len(models) and (seeds is None or len(seeds) == len(s))
        arr = models if isinstance(models, C.Array) else (C.c_void_p * len(models))(*models)
        self._ck(self.lib.vfgs_hip_add_grain_sp_frame_list_models_to_planar_dev(s, d, arr, self.seed_list(seeds), len(s), width, height, stride,
                                                                                uv_stride, dst_stride, dst_cstride, sample_shift, stream))

    def seed_segments(self, seeds, first_bit, seg_words):
        """What a seeded launch uploads (host only): a list of len(seeds) lists of seg_words registers (include/vfgs_hip.h)."""
        out = (C.c_uint32 * (len(seeds) * seg_words))()
        self._ck(self.lib.vfgs_hip_seed_segments(self.seed_list(seeds), len(seeds), first_bit, seg_words, out))
        return [list(out[f * seg_words:(f + 1) * seg_words]) for f in range(len(seeds))]

    def seeded_stream_stats(self):
        out = (C.c_uint64 * 4)()
        self.lib.vfgs_hip_get_seeded_stream_stats(out)
        return {"images_built": out[0], "image_words": out[1], "host_waits": out[2], "last_launch_used_it": bool(out[3])}

    def seed_state(self):
        out = (C.c_uint32 * 4)()
        self.lib.vfgs_hip_get_seed_state(out)
        return tuple(out)

    def luts(self, c):
        """(scale LUT, pattern LUT) of component c as bytes."""
        a, b = C.create_string_buffer(256), C.create_string_buffer(256)
        self._ck(self.lib.vfgs_hip_get_luts(c, a, b))
        return a.raw, b.raw

    def params(self):
        out = (C.c_int * 8)()
        self.lib.vfgs_hip_get_params(out)
        return dict(zip(("scale_shift", "bs", "ymin", "ymax", "cmin", "cmax", "csubx", "csuby"), out))

    def set_chroma_mix(self, c, luma_mult, chroma_mult, offset):
        """Luma / chroma mix of component c's (1 = Cb, 2 = Cr) look-up index (include/vfgs_hip.h)."""
        self._ck(self.lib.vfgs_hip_set_chroma_mix(c, luma_mult, chroma_mult, offset))

    def clear_chroma_mix(self):
        self.lib.vfgs_hip_clear_chroma_mix()

    def chroma_mix(self, c):
        """(luma_mult, chroma_mult, offset, active) of component c."""
        out = (C.c_int * 4)()
        self._ck(self.lib.vfgs_hip_get_chroma_mix(c, out))
        return tuple(out)

    def line_lookahead(self, enable):
        self.lib.vfgs_hip_line_lookahead(1 if enable else 0)

    def declare_frame(self, Y, U, V, width, height, stride, cstride):
        self._ck(self.lib.vfgs_hip_declare_frame(Y, U, V, width, height, stride, cstride))

    def add_grain_frames_host(self, Ys, Us, Vs, width, height, stride, cstride):
        """Frames in host memory (lists of plane addresses), pipelined upload / kernel / download."""
        n = len(Ys)
        assert len(Us) == n and len(Vs) == n
        arr = lambda ps: (C.c_void_p * n)(*ps)
        self._ck(self.lib.vfgs_hip_add_grain_frames_host(arr(Ys), arr(Us), arr(Vs), n, width, height, stride, cstride))

    def host_pipe(self, width, height, stride, cstride, dst_stride=0, dst_cstride=0, dst8=False, slots=0):
        """A pipe for pictures in host memory that arrive one at a time, each with its own model and seed (include/vfgs_hip.h:
        vfgs_hip_host_pipe_open): an object with submit(src, dst=None, model=None, seed=None) -> ticket, wait(ticket) and close(), also a
        context manager.  dst_stride = dst_cstride = 0: in place; dst8: planar 8-bit destination of a 10- or 12-bit pipe; slots: pictures
        in flight (0 = 3, else 2..8)."""
        return HostPipe(self, HostPipeDesc(width, height, stride, cstride, dst_stride, dst_cstride, 1 if dst8 else 0, slots))

    def host_alloc(self, nbytes):
        p = self.lib.vfgs_hip_host_alloc(nbytes)
        if not p:
            raise VfgsHipError(f"vfgs_hip_host_alloc({nbytes}): {self.lib.vfgs_hip_last_error_string().decode()}")
        return p

    def host_free(self, p):
        self.lib.vfgs_hip_host_free(p)

    def stream_stats(self):
        out = (C.c_uint64 * 4)()
        self.lib.vfgs_hip_get_stream_stats(out)
        return {"refills_in_stream": out[0], "windows_built_ahead": out[1], "switches_to_built_ahead": out[2], "window_words": out[3]}

    def stripe_stream_stats(self):
        out = (C.c_uint64 * 4)()
        self.lib.vfgs_hip_get_stripe_stream_stats(out)
        return {"built_in_stream": out[0], "built_ahead": out[1], "switches_to_built_ahead": out[2], "last_launch_used_it": bool(out[3])}

    def overlap_begin(self, stream=0):
        self._ck(self.lib.vfgs_hip_overlap_begin(stream))

    def overlap_end(self, stream=0):
        self._ck(self.lib.vfgs_hip_overlap_end(stream))

    def init_devices(self, devices):
        """Host-memory frames and stripes are split over these devices from now on (devices[0] stays the library's device)."""
        arr = (C.c_int * len(devices))(*devices)
        self._ck(self.lib.vfgs_hip_init_devices(arr, len(devices)))

    def last_launch_info(self):
        """What the most recent grain launch dispatched (dict), or None before the first launch."""
        li = LaunchInfo()
        if self.lib.vfgs_hip_last_launch_info(C.byref(li)):
            return None
        d = {k: getattr(li, k) for k, _ in LaunchInfo._fields_ if k not in ("rows_per_wave", "positions_per_row", "kernel")}
        d["rows_per_wave"] = list(li.rows_per_wave)
        d["positions_per_row"] = list(li.positions_per_row)
        d["kernel"] = li.kernel.decode()
        return d

    def device_info(self):
        cu, lds, clk = C.c_int(), C.c_int(), C.c_int()
        name = C.create_string_buffer(128)
        self._ck(self.lib.vfgs_hip_device_info(C.byref(cu), C.byref(lds), C.byref(clk), name, 128))
        return {"cu_count": cu.value, "lds_per_cu": lds.value, "clock_khz": clk.value, "name": name.value.decode()}


class HostPipe:
    """An open vfgs_hip_host_pipe (VfgsHip.host_pipe).  src / dst: (Y, U, V) HOST addresses of line 0 of the planes; they stay valid and
    untouched until wait(ticket) has returned.  model: a handle of model_capture / models_from_* (None: the programmed state as it is
    now), which may be released as soon as submit returns; seed: what vfgs_set_seed would get (None: the running seed sequence)."""

    def __init__(self, hip, desc):
        self._hip, self.desc = hip, desc
        h = C.c_void_p()
        hip._ck(hip.lib.vfgs_hip_host_pipe_open(C.byref(desc), C.byref(h)))
        self.handle = h.value

    def submit(self, src, dst=None, model=None, seed=None):
        s = FramePtrs(*src)
        d = None if dst is None else C.byref(FramePtrs(*dst))
        sd = None if seed is None else C.byref(C.c_uint32(int(seed) & 0xFFFFFFFF))
        t = C.c_uint64(0)
        self._hip._ck(self._hip.lib.vfgs_hip_host_pipe_submit(self.handle, C.byref(s), d, model, sd, C.byref(t)))
        return t.value

    def wait(self, ticket):
        self._hip._ck(self._hip.lib.vfgs_hip_host_pipe_wait(self.handle, ticket))

    def close(self):
        """Drains the pipe and frees its ring; a second close is a no-op."""
        if self.handle is not None:
            h, self.handle = self.handle, None
            self._hip._ck(self._hip.lib.vfgs_hip_host_pipe_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
