"""ctypes binding of libpmp_hip.so (C ABI: include/pmp.h).  No torch types cross this boundary: only raw
pointers and sizes.  The library is built in-tree by `make -C pmp_vvc_tip2023_amd/csrc` (see __graft_entry__.build)."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpmp_hip.so")
HOSTASAN_LIB_PATH = os.path.join(_HERE, "libpmp_hostasan.so")      # make hostasan: host-only units under ASan/UBSan (tests only)

PMP_LUMA, PMP_CHROMA = 0, 1
PMP_RECORD_BYTES = 1344
PMP_MSBT_LEAF_BUDGET = 4096
PMP_VAL_NSTATS = 20
PMP_LOSS_NTERMS = 13
PMP_CONF_MAPS, PMP_CONF_CLASSES, PMP_CONF_NCOUNTS = 7, 5, 175
PMP_MSBT_INCONSISTENT, PMP_MSBT_QT_DEEP, PMP_MSBT_BUDGET = 1, 2, 4
NET_IDS = {"Luma_Q": 0, "Luma_MSBD": 1, "Chroma_Q": 2, "Chroma_MSBD": 3}
ERRORS = {-1: "PMP_E_INVALID", -2: "PMP_E_HIP", -3: "PMP_E_NOWEIGHTS", -4: "PMP_E_IO", -5: "PMP_E_NOMEM", -6: "PMP_E_NODEVICE", -7: "PMP_E_RANGE"}


class PmpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "PMP_E_?"), code, msg))
        self.code = code


class TensorDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ndim", C.c_int), ("shape", C.c_int * 4), ("offset", C.c_int64)]


class PartitionParams(C.Structure):
    """pmp_partition_params: Map_to_Partition's lamb1..lamb5 (Map2Partition.py:100) and th_round's thd (:105)."""
    _fields_ = [("lamb", C.c_double * 5), ("thd", C.c_float)]


class LossParams(C.Structure):
    """pmp_loss_params: Train_QBD's --lambq, --lambb0..2, --lambd0..2, --lambresb0..2 (Train_QBD.py:448-457)."""
    _fields_ = [("lambq", C.c_double), ("lambb", C.c_double * 3), ("lambd", C.c_double * 3), ("lambresb", C.c_double * 3)]


class RbShape(C.Structure):
    """pmp_rb_shape: one ResidualBlock of pmp_resblock_forward / _backward."""
    _fields_ = [("n", C.c_int), ("h", C.c_int), ("w", C.c_int), ("cin", C.c_int), ("cout", C.c_int), ("k", C.c_int)]


PMP_TRUNK_MAX_BLOCKS = 8


class TrunkShape(C.Structure):
    """pmp_trunk_shape: a chain of ResidualBlocks (block i: cout[i-1] or cin -> cout[i], k[i]) and an optional 2x2 max-pool."""
    _fields_ = [("n", C.c_int), ("h", C.c_int), ("w", C.c_int), ("cin", C.c_int), ("nblocks", C.c_int),
                ("cout", C.c_int * PMP_TRUNK_MAX_BLOCKS), ("k", C.c_int * PMP_TRUNK_MAX_BLOCKS), ("pool", C.c_int)]


def trunk_shape(shape):
    """(n, h, w, cin, [(cout, k), ...], pool) -> TrunkShape (a TrunkShape passes through).  More blocks than the struct holds keep
    their count, so that the library refuses the shape; their channels have no place to go."""
    if isinstance(shape, TrunkShape):
        return shape
    n, h, w, cin, blocks, pool = shape
    s = TrunkShape(int(n), int(h), int(w), int(cin), len(blocks))
    for i, (cout, k) in enumerate(blocks[:PMP_TRUNK_MAX_BLOCKS]):
        s.cout[i], s.k[i] = int(cout), int(k)
    s.pool = int(pool)
    return s


class StemShape(C.Structure):
    """pmp_stem_shape: a net's first layer, x [n][cin][h + k/2][w + k/2] -> y [n][32][h][w]; split 1: the MTT nets' three convolutions."""
    _fields_ = [("n", C.c_int), ("h", C.c_int), ("w", C.c_int), ("cin", C.c_int), ("k", C.c_int), ("split", C.c_int)]


def stem_shape(shape):
    """(n, h, w, cin, k, split) -> StemShape (a StemShape passes through)."""
    return shape if isinstance(shape, StemShape) else StemShape(*(int(v) for v in shape))


class HeadShape(C.Structure):
    """pmp_head_shape: an MTT net's head, x [n][cin][h][w] -> y [n][cout][h][w] and, with up_y, att [n][1+cout][up_y h][up_y w]."""
    _fields_ = [("n", C.c_int), ("h", C.c_int), ("w", C.c_int), ("cin", C.c_int), ("cout", C.c_int), ("up_q", C.c_int), ("up_y", C.c_int)]


def head_shape(shape):
    """(n, h, w, cin, cout, up_q, up_y) -> HeadShape (a HeadShape passes through)."""
    return shape if isinstance(shape, HeadShape) else HeadShape(*(int(v) for v in shape))


class QtailShape(C.Structure):
    """pmp_qtail_shape: a QT net's tail, x4 [n][64][h][w] -> x9 [n][8][h/2][w/2]."""
    _fields_ = [("n", C.c_int), ("h", C.c_int), ("w", C.c_int)]


def qtail_shape(shape):
    """(n, h, w) -> QtailShape (a QtailShape passes through)."""
    return shape if isinstance(shape, QtailShape) else QtailShape(*(int(v) for v in shape))


class BatchSrc(C.Structure):
    """pmp_batch_src: the whole data set on the device (pmp_batch_gather_device); u, v both set = chroma; absent labels NULL."""
    _fields_ = [(k, C.c_void_p) for k in ("y", "u", "v", "qt8", "msbt", "msdire")] + [("count", C.c_int64)]


class BatchDst(C.Structure):
    """pmp_batch_dst: the outputs of pmp_batch_gather_device for n rows, each NULL where it is not asked for."""
    _fields_ = [(k, C.c_void_p) for k in ("x", "qt_f", "qt8", "msbt", "msdire")]


class AdamParams(C.Structure):
    """pmp_adam_params: torch.optim.Adam's lr, betas and eps."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


class GuardParams(C.Structure):
    """pmp_guard_params: max_norm 0 = no clipping; skip_nonfinite = a step with a NaN or inf gradient writes nothing."""
    _fields_ = [("max_norm", C.c_double), ("skip_nonfinite", C.c_int)]


class GuardRecord(C.Structure):
    """pmp_guard_record, 32 bytes in device memory: action bit 0 = skip, bit 1 = clip."""
    _fields_ = [("sumsq", C.c_double), ("norm", C.c_double), ("nonfinite", C.c_int64), ("coef", C.c_float), ("action", C.c_uint32)]


class GuardState(C.Structure):
    """pmp_guard_state, 48 bytes in device memory: the running counters of pmp_grad_guard_device."""
    _fields_ = [(k, C.c_int64) for k in ("steps", "skipped", "clipped", "run", "max_run")] + [("max_norm", C.c_double)]


PMP_BATCH_MAX = 65536
PMP_ADAM_TABLE = 96
PMP_SELECT_MAX_FLAGS = 64
PMP_GRAD_SUM_MAX = 64


def pointer_array(ptrs, count):
    """A host array of `count` device pointers (None = NULL) for the C ABI; None stays None."""
    if ptrs is None:
        return None
    ptrs = list(ptrs)
    if len(ptrs) != count:
        raise ValueError("expected %d pointers, got %d" % (count, len(ptrs)))
    return (C.c_void_p * count)(*ptrs)


# name -> (restype, argtypes); every symbol declared in include/pmp.h
_VP, _I, _I64, _U32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32
SIGNATURES = {
    "pmp_version": (C.c_char_p, []),
    "pmp_last_error": (C.c_char_p, [_VP]),
    "pmp_create": (_I, [_I, C.POINTER(_VP)]),
    "pmp_destroy": (_I, [_VP]),
    "pmp_trim": (_I, []),
    "pmp_set_stream": (_I, [_VP, _VP]),
    "pmp_synchronize": (_I, [_VP]),
    "pmp_set_chunk": (_I, [_VP, _I]),
    "pmp_set_overlap": (_I, [_VP, _I]),
    "pmp_get_workspace_bytes": (_I64, [_VP]),
    "pmp_set_precision": (_I, [_VP, _I]),
    "pmp_get_precision": (_I, [_VP]),
    "pmp_set_saturation_policy": (_I, [_VP, _I]),
    "pmp_get_saturation": (_I, [_VP]),
    "pmp_get_saturation_reruns": (_I64, [_VP]),
    "pmp_clear_saturation": (_I, [_VP]),
    "pmp_load_weights": (_I, [_VP, _I, _I, _VP, C.POINTER(TensorDesc), _I]),
    "pmp_load_weights_file": (_I, [_VP, _I, _I, C.c_char_p]),
    "pmp_has_weights": (_I, [_VP, _I, _I]),
    "pmp_weights_fingerprint": (_I, [_VP, _I, _I, C.POINTER(C.c_uint64)]),
    "pmp_fingerprint_tensors": (_I, [_VP, C.POINTER(TensorDesc), _I, C.POINTER(C.c_uint64)]),
    "pmp_debug_read_weights_file": (_I, [C.c_char_p, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I64), C.POINTER(C.c_double)]),
    "pmp_infer": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I64, _VP, _VP, _VP]),
    "pmp_infer_device": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I64, _VP, _VP, _VP]),
    "pmp_infer_q": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I64, _VP]),
    "pmp_infer_q_device": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I64, _VP]),
    "pmp_postprocess": (_I, [_VP, _I, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP]),
    "pmp_postprocess_device": (_I, [_VP, _I, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP]),
    "pmp_set_partition_params": (_I, [_VP, _I, C.POINTER(PartitionParams)]),
    "pmp_get_partition_params": (_I, [_VP, _I, C.POINTER(PartitionParams)]),
    "pmp_parse_partition_params": (_I, [C.c_char_p, C.POINTER(PartitionParams)]),
    "pmp_infer_postprocess": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pmp_infer_postprocess_device": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pmp_postprocess_records_device": (_I, [_VP, _I, _VP, _VP, _VP, _I64, _VP]),
    "pmp_infer_postprocess_records_device": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I64, _VP]),
    "pmp_cut_blocks": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP]),
    "pmp_cut_blocks_device": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP]),
    "pmp_msbt_labels": (_I, [_VP, _I, _VP, _VP, _VP, _I64, _VP, _VP]),
    "pmp_msbt_labels_device": (_I, [_VP, _I, _VP, _VP, _VP, _I64, _VP, _VP]),
    "pmp_label_partition": (_I, [_VP, _I, _VP, _VP, _VP, _I64, _VP, _VP, _VP]),
    "pmp_label_partition_device": (_I, [_VP, _I, _VP, _VP, _VP, _I64, _VP, _VP, _VP]),
    "pmp_label_partition_records_device": (_I, [_VP, _I, _VP, _VP, _VP, _I64, _VP, _VP]),
    "pmp_val_stats": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "pmp_val_stats_device": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _VP]),
    "pmp_val_confusion": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "pmp_val_confusion_device": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _VP]),
    "pmp_parse_loss_params": (_I, [C.c_char_p, C.POINTER(LossParams)]),
    "pmp_train_loss": (_I, [_VP, _I, _I, C.POINTER(LossParams), _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP]),
    "pmp_train_loss_device": (_I, [_VP, _I, _I, C.POINTER(LossParams), _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP]),
    "pmp_resblock_forward": (_I, [_VP, C.POINTER(RbShape)] + [_VP] * 6),
    "pmp_resblock_forward_device": (_I, [_VP, C.POINTER(RbShape)] + [_VP] * 6),
    "pmp_resblock_backward": (_I, [_VP, C.POINTER(RbShape)] + [_VP] * 11),
    "pmp_resblock_backward_device": (_I, [_VP, C.POINTER(RbShape)] + [_VP] * 11),
    "pmp_trunk_saved_bytes": (_I64, [C.POINTER(TrunkShape)]),
    "pmp_trunk_forward_device": (_I, [_VP, C.POINTER(TrunkShape), _VP, _VP, _VP, _VP]),
    "pmp_trunk_backward_device": (_I, [_VP, C.POINTER(TrunkShape), _VP, _VP, _VP, _VP, _VP]),
    "pmp_trunk_unpack_device": (_I, [_VP, C.POINTER(TrunkShape), _VP, _I, _VP]),
    "pmp_qtail_saved_bytes": (_I64, [C.POINTER(QtailShape)]),
    "pmp_qtail_forward_device": (_I, [_VP, C.POINTER(QtailShape), _VP, _VP, _VP, _VP]),
    "pmp_qtail_backward_device": (_I, [_VP, C.POINTER(QtailShape), _VP, _VP, _VP, _VP, _VP]),
    "pmp_qtail_unpack_device": (_I, [_VP, C.POINTER(QtailShape), _VP, _I, _VP]),
    "pmp_stem_forward_device": (_I, [_VP, C.POINTER(StemShape), _VP, _VP, _VP, _VP]),
    "pmp_stem_backward_device": (_I, [_VP, C.POINTER(StemShape)] + [_VP] * 7),
    "pmp_head_forward_device": (_I, [_VP, C.POINTER(HeadShape)] + [_VP] * 7),
    "pmp_head_backward_device": (_I, [_VP, C.POINTER(HeadShape)] + [_VP] * 9),
    "pmp_gate_forward_device": (_I, [_VP, _I64, _VP, _VP, _VP]),
    "pmp_gate_backward_device": (_I, [_VP, _I64] + [_VP] * 6),
    "pmp_batch_gather_device": (_I, [_VP, C.POINTER(BatchSrc), _VP, _I64, C.POINTER(BatchDst), _VP]),
    "pmp_adam_step_device": (_I, [_VP, C.POINTER(AdamParams), _I, _VP, _VP, _VP, _VP, C.POINTER(_I64), _I64]),
    "pmp_grad_guard_scratch_bytes": (_I64, [_I, C.POINTER(_I64)]),
    "pmp_grad_guard_device": (_I, [_VP, C.POINTER(GuardParams), _I, _VP, C.POINTER(_I64), _VP, _VP, _VP]),
    "pmp_adam_step_guarded_device": (_I, [_VP, C.POINTER(AdamParams), _I, _VP, _VP, _VP, _VP, C.POINTER(_I64), _I64, _VP]),
    "pmp_grad_bucket_floats": (_I64, [_I, C.POINTER(_I64), C.POINTER(_I64)]),
    "pmp_grad_pack_device": (_I, [_VP, _I, _VP, C.POINTER(_I64), _VP]),
    "pmp_grad_sum_device": (_I, [_VP, _I, _VP, _I64, _VP]),
    "pmp_select_rows_device": (_I, [_VP, _VP, _I, _I, _VP, _I, _I64, _I64, _VP, _VP]),
    "pmp_gather_rows_device": (_I, [_VP, _VP, _I64, _I64, _VP, _I64, _VP, _VP]),
    "pmp_infer_msbd": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _I64, _VP, _VP]),
    "pmp_infer_msbd_device": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _I64, _VP, _VP]),
    "pmp_read_depth_dump": (_I, [C.c_char_p, _I, _I, _I, _I, _VP, _VP, _VP, C.POINTER(_I64)]),
    "pmp_write_partition_file": (_I, [C.c_char_p, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "pmp_write_partition_binary": (_I, [C.c_char_p, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "pmp_tile_partition_maps": (_I, [_I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pmp_format_partition_text": (_I64, [_I, _I, _I, _VP, _VP, _VP, _VP, _VP, _I64]),
    "pmp_format_partition_rows": (_I64, [_I, _I, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "pmp_format_partition_rows_records": (_I64, [_I, _I, _VP, _VP, _I64, _VP]),
    "pmp_tile_partition_rows_records": (_I, [_I, _I, _VP, _VP, _VP, _VP, _VP]),
    "pmp_ktime_enable": (_I, [_VP, _U32]),
    "pmp_ktime_classes": (_I, []),
    "pmp_ktime_name": (C.c_char_p, [_I]),
    "pmp_ktime_get": (_I, [_VP, _I, C.POINTER(_I64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pmp_debug_set_conv_variant": (_I, [_I]),
    "pmp_debug_set_winograd": (_I, [_VP, _I]),
    "pmp_debug_set_fusion": (_I, [_VP, _I]),
    "pmp_debug_set_activation_scales": (_I, [_VP, _I]),
    "pmp_debug_activation_report": (_I, [_VP, _I, _I, C.POINTER(_I), C.POINTER(C.c_float), C.c_char_p, _I64]),
    "pmp_debug_set_taps": (_I, [_VP, _I]),
    "pmp_debug_get_tap": (_I64, [_VP, C.c_char_p, _VP, _I64, C.POINTER(_I), C.POINTER(_I)]),
    "pmp_debug_poison_workspace": (_I, [_VP, _I]),
    "pmp_debug_pack_f16x3": (C.c_int64, [C.POINTER(C.c_float), _I, _I, _I, C.POINTER(C.c_uint16), C.c_int64, C.POINTER(C.c_int)]),
    "pmp_debug_conv_bench": (_I, [_VP, _I, _I, _I, _I, _I, _I, _I] + [C.POINTER(C.c_double)] * 4),
    "pmp_debug_run_resblock": (_I, [_VP, _VP] + [C.POINTER(C.c_float)] * 5 + [C.POINTER(_I), C.c_char_p, _I64]),
}

_lib = None


def open_library(path, subset=False):
    """dlopen a build of the C ABI and type its entry points.  subset=True accepts a library that exports only some of
    include/pmp.h (the host-only sanitizer build); the product library must export all of it."""
    if not os.path.isfile(path):
        raise ImportError("%s is missing - build it with `make -C %s` (or __graft_entry__.build())"
                          % (path, os.path.join(_HERE, "csrc")))
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        if subset and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def _torch_first():
    """The PyTorch-ROCm wheel bundles its own libamdhip64 with the same soname as /opt/rocm's, so whichever copy is loaded first
    serves the whole process.  With ours first, torch finds "No HIP GPUs" (seen on the GPU pool: the driver then silently kept its
    blocks on the host).  Where torch is installed - it is the device allocator of the driver, bench and tests - it goes first."""
    import sys
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass


def load(path=None):
    """Load libpmp_hip.so (or, for tools/ and tests, the build at `path` - before anything else loaded the library).
    Fails loudly when the extension has not been built: there is no fallback path."""
    global _lib
    if _lib is None:
        _torch_first()
        _lib = open_library(path or LIB_PATH)
    elif path is not None and os.path.abspath(path) != os.path.abspath(_lib._name):
        raise RuntimeError("a different build of the library is already loaded: %s" % _lib._name)
    return _lib


def check(rc, ctx=None):
    if rc < 0:
        msg = load().pmp_last_error(ctx)
        raise PmpError(int(rc), msg.decode() if msg else "")
    return rc
