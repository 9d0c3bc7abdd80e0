"""Host-side mirror of the reference's hot-path functions, running on libpmp_hip.so.

Same names and argument meaning as the reference so callers (and the parity tests) read alike:

    reference                                           here
    Metrics.inference_pre_QBD(loader, Net_Q, Net_BD)    Engine.inference_pre_QBD(comp, qp, block_y[, block_u, block_v])
    Metrics.seq_post_process(qt, bt, dire, comp, ...)   Engine.seq_post_process(qt, bt, dire, comp, sub_numfrm, width, height, save_path)
    Inference_QBD.output_block_yuv(...)                 Engine.output_block_yuv(y, u, v, bitdepth)
    Inference_QBD.load_pretrain_model(net, path)        Engine.load_pretrain_model(net_name, qp, weights)
    GenMSBtMap.gen_seq_sub_map(qt, bt, dire, is_luma)   Engine.gen_seq_sub_map(qt, bt, dire, is_luma)   (training labels)
    GenMSBtMap.map_to_parititon(qt, bt, dire, cf)       Engine.label_partition(qt, bt, dire, cf)        (all blocks at once)
    GenMSBtMap.get_sequence_partition_for_VTM(...)      Engine.label_partition_for_VTM(...)             (labels -> PartitionMat file)
    Metrics.validation_QBD(loader, Net_Q, Net_BD, qp)   Engine.validation_QBD(comp, qp, blocks, qt8, msbt, msdire, batch_size)
    Metrics.pre_validation(loader, Net, predID, qp)     Engine.pre_validation(comp, qp, pred_id, blocks, qt8[, msbt, msdire], batch_size)
    Train_QBD.loss_func_QBD / loss_func_MSBD / L1_Loss  Engine.train_loss(comp, qp, ...)  (+ gradients; torch: train_loss.py)
    CreateDataSet.output_block_partition_map(...)       output_block_partition_map(...)                 (module level, host only)

numpy arrays in/out for the host API; the *_device methods take raw device pointers (ints), e.g. torch
tensors' .data_ptr(), and run asynchronously on the engine's stream.  There is no CPU fallback: constructing an
Engine without a gfx950 device raises PmpError(PMP_E_NODEVICE).
"""
import ctypes as C

import numpy as np

from . import _lib, validation
from . import weights as W
from .validation import CONF_MAPS, VAL_ELEMS, _fit, _logit_label_arrays, confusion_summary, validation_numbers  # noqa: F401 (kept importable from here)

COMP_ID = {"Luma": _lib.PMP_LUMA, "Chroma": _lib.PMP_CHROMA}
PARAM_KEYS = ("lamb1", "lamb2", "lamb3", "lamb4", "lamb5", "thd")
DEFAULT_PARTITION_PARAMS = {"lamb1": 0.7, "lamb2": 0.7, "lamb3": 1.5, "lamb4": 0.3, "lamb5": 0.7, "thd": 0.5}   # Map2Partition.py:100,105


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _u8(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint8)


class Engine:
    def __init__(self, device=0, weight_dir=None, chunk=None, allow_synthetic_mtt=False):
        """allow_synthetic_mtt: let load() fall back to the synthetic MTT-net weights when a *_BD_* file is missing (tests,
        bench, smoke); off by default - a production run with a missing model file must fail (Inference_QBD.py:219-222)."""
        self.lib = _lib.load()
        self.allow_synthetic_mtt = bool(allow_synthetic_mtt)
        self.h = C.c_void_p()
        _lib.check(self.lib.pmp_create(int(device), C.byref(self.h)))
        self.device = device
        self.weight_dir = weight_dir
        self.provenance = {}
        self.stream_ptr = 0
        if chunk:
            self.set_chunk(chunk)

    # ------------------------------------------------------------------------------------------ plumbing
    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.pmp_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        return _lib.check(rc, self.h)

    def set_stream(self, hip_stream_ptr):
        self._ck(self.lib.pmp_set_stream(self.h, C.c_void_p(hip_stream_ptr or 0)))
        self.stream_ptr = hip_stream_ptr or 0           # what the engine runs on now (0: the context's own stream)

    def set_chunk(self, blocks):
        self._ck(self.lib.pmp_set_chunk(self.h, int(blocks)))

    def set_overlap(self, on):
        """Two chunks of a large call in flight on two streams (include/pmp.h: pmp_set_overlap)."""
        self._ck(self.lib.pmp_set_overlap(self.h, 1 if on else 0))

    def workspace_bytes(self):
        return int(self.lib.pmp_get_workspace_bytes(self.h))

    def set_precision(self, mode):
        """'f16x3' (default; 2-term fp16 split, 3 MFMA products), 'bf16x6' (3-term bf16 split, 6 products) - both
        fp32-equivalent - or 'fp32' (exact fp32 MFMA)."""
        self._ck(self.lib.pmp_set_precision(self.h, {"fp32": 0, "f32": 0, "bf16x6": 1, "f16x3": 2}[mode]))

    def set_fusion(self, on):
        """f16x3 launch fusion (include/pmp.h: pmp_debug_set_fusion; bit-identical results either way): True / 1 = all (default), False / 0 =
        launch per layer, 2 = only the 16x16 tails (chain16.hip), 3 = only the 32x32 ResidualBlocks (rbfuse32.hip)."""
        self._ck(self.lib.pmp_debug_set_fusion(self.h, int(on)))

    def get_precision(self):
        return {0: "fp32", 1: "bf16x6", 2: "f16x3"}[self.lib.pmp_get_precision(self.h)]

    def set_saturation_policy(self, policy):
        """f16x3 range guard (include/pmp.h): 'rerun' (default: a call whose activations left the fp16 range is run again on
        the exact fp32 MFMA datapath), 'error' (PMP_E_RANGE instead) or 'ignore' (no check, fully asynchronous device calls)."""
        self._ck(self.lib.pmp_set_saturation_policy(self.h, {"rerun": 0, "error": 1, "ignore": 2}[policy]))

    def saturated(self):
        """True if any inference call since clear_saturation() drove an f16x3 activation beyond +-65504."""
        return bool(self._ck(self.lib.pmp_get_saturation(self.h)))

    def saturation_reruns(self):
        return int(self.lib.pmp_get_saturation_reruns(self.h))

    def clear_saturation(self):
        self._ck(self.lib.pmp_clear_saturation(self.h))

    def set_activation_scales(self, on):
        """f16x3: use the calibrated activation scales of the MTT nets (default) or exponents of zero (include/pmp.h; the range-guard tests)."""
        self._ck(self.lib.pmp_debug_set_activation_scales(self.h, 1 if on else 0))

    def activation_report(self, comp, qp):
        """f16x3 activation scales of the MTT net of (comp, qp) and the calibration record behind them (include/pmp.h):
        {"exps": [e0..e4], "seg_amax": [..5..], "tensors": [(name, segment, max |value|), ...]}.  Loads the pair if necessary."""
        self.load(comp, qp)
        exps = (C.c_int * 5)()
        amax = (C.c_float * 5)()
        buf = C.create_string_buffer(16384)
        n = self._ck(self.lib.pmp_debug_activation_report(self.h, COMP_ID[comp], int(qp), exps, amax, buf, len(buf)))
        rows = [ln.split() for ln in buf.value.decode().splitlines()]
        assert len(rows) == n
        return {"exps": list(exps), "seg_amax": list(amax), "tensors": [(r[0], int(r[1]), float(r[2])) for r in rows]}

    def synchronize(self):
        self._ck(self.lib.pmp_synchronize(self.h))

    # ------------------------------------------------------------------------------------------ Map2Partition thresholds
    def set_partition_params(self, comp, **kw):
        """Thresholds of the post-processing search for `comp` (include/pmp.h: pmp_set_partition_params), named as in the reference:
        lamb1..lamb5 (Map_to_Partition, Map2Partition.py:100) and thd (th_round, :105).  Keys not given keep their CURRENT value;
        no keys at all restores the reference's defaults.  Outside the accepted domain: PmpError(PMP_E_INVALID), the old set stays.
        Calls already enqueued keep the set they were enqueued with."""
        if not kw:
            self._ck(self.lib.pmp_set_partition_params(self.h, COMP_ID[comp], None))
            return
        p = self._params(comp)
        for k, v in kw.items():
            if k == "thd":
                p.thd = float(v)
            elif k in PARAM_KEYS[:5]:
                p.lamb[PARAM_KEYS.index(k)] = float(v)
            else:
                raise TypeError("set_partition_params: unknown threshold %r (lamb1..lamb5, thd)" % k)
        self._ck(self.lib.pmp_set_partition_params(self.h, COMP_ID[comp], C.byref(p)))

    def get_partition_params(self, comp):
        """{'lamb1': .., ..., 'lamb5': .., 'thd': ..} in force for `comp` (thd as stored: a float32 value)."""
        return params_dict(self._params(comp))

    def _params(self, comp):
        p = _lib.PartitionParams()
        self._ck(self.lib.pmp_get_partition_params(self.h, COMP_ID[comp], C.byref(p)))
        return p

    # ------------------------------------------------------------------------------------------ weights
    def load_pretrain_model(self, net, qp, tensors):
        """net in {Luma_Q, Luma_MSBD, Chroma_Q, Chroma_MSBD}; tensors {state_dict name: float32 ndarray}."""
        names = list(tensors.keys())
        arrs = [np.ascontiguousarray(tensors[k], dtype=np.float32).ravel() for k in names]
        blob = np.concatenate(arrs) if arrs else np.zeros(0, np.float32)
        descs = (_lib.TensorDesc * len(names))()
        off = 0
        keep = []
        for i, k in enumerate(names):
            shp = tuple(np.shape(tensors[k]))
            kb = k.encode()
            keep.append(kb)
            descs[i].name = kb
            descs[i].ndim = len(shp)
            for j in range(4):
                descs[i].shape[j] = int(shp[j]) if j < len(shp) else 0
            descs[i].offset = off
            off += arrs[i].size
        self._ck(self.lib.pmp_load_weights(self.h, _lib.NET_IDS[net], int(qp), _ptr(blob), descs, len(names)))

    def has_weights(self, net, qp):
        return bool(self.lib.pmp_has_weights(self.h, _lib.NET_IDS[net], int(qp)))

    def check_available(self, comp, qp, kinds=("Q", "MSBD")):
        """Raise FileNotFoundError now if load(comp, qp) would: the driver loads weights lazily, next to the GPU's work, but a
        missing model file must stop the job before any output (Inference_QBD.py:219-222).  kinds = ("Q",): what load_q needs."""
        for kind in kinds:
            net = "%s_%s" % (comp, kind)
            if not self.has_weights(net, qp):
                W.find_net_weights(net, qp, self.weight_dir, allow_synthetic=self.allow_synthetic_mtt)

    def load_q(self, comp, qp, q_weights=None):
        """Load the QT net of (comp, qp) alone: all that infer_q and pre_validation(pred_id=0) need.  No *_BD_* file is looked for."""
        self.load(comp, qp, q_weights=q_weights, kinds=("Q",))

    def load(self, comp, qp, q_weights=None, msbd_weights=None, kinds=("Q", "MSBD")):
        """Load both nets of (comp, qp); missing dicts are resolved by weights.load_net_weights().  kinds: the nets to load."""
        for kind, given in (("Q", q_weights), ("MSBD", msbd_weights)):
            if kind not in kinds:
                continue
            net = "%s_%s" % (comp, kind)
            if given is None:
                if self.has_weights(net, qp):
                    continue
                kind, path = W.find_net_weights(net, qp, self.weight_dir, allow_synthetic=self.allow_synthetic_mtt)
                if kind == "pmpw":      # the library's own reader: no copies through Python (pmp_load_weights_file)
                    self._ck(self.lib.pmp_load_weights_file(self.h, _lib.NET_IDS[net], int(qp), path.encode()))
                    self.provenance[(net, qp)] = path
                    continue
                given, src = W.load_net_weights(net, qp, self.weight_dir, allow_synthetic=self.allow_synthetic_mtt)
            else:
                src = "caller"
            self.load_pretrain_model(net, qp, given)
            self.provenance[(net, qp)] = src

    # ------------------------------------------------------------------------------------------ host API
    def inference_pre_QBD(self, comp, qp, block_y, block_u=None, block_v=None):
        """Metrics.py:387-419.  block_y u8[N,68,68] (+ block_u/v u8[N,34,34] for Chroma)
        -> qt f32[N,1,8,8], bt f32[N,3,16,16], dire f32[N,3,16,16]."""
        by, bu, bv = _u8(block_y), _u8(block_u), _u8(block_v)
        n = self._check_blocks(comp, by, bu, bv)
        self.load(comp, qp)
        qt = np.empty((n, 1, 8, 8), np.float32); bt = np.empty((n, 3, 16, 16), np.float32); dire = np.empty((n, 3, 16, 16), np.float32)
        self._ck(self.lib.pmp_infer(self.h, COMP_ID[comp], int(qp), _ptr(by), _ptr(bu), _ptr(bv), n, _ptr(qt), _ptr(bt), _ptr(dire)))
        return qt, bt, dire

    def infer_q(self, comp, qp, block_y, block_u=None, block_v=None):
        """pmp_infer_q: the QT net of (comp, qp) alone -> qt f32[N,1,8,8], the qt of inference_pre_QBD bit for bit.  Loads the QT net only."""
        by, bu, bv = _u8(block_y), _u8(block_u), _u8(block_v)
        n = self._check_blocks(comp, by, bu, bv)
        self.load_q(comp, qp)
        qt = np.empty((n, 1, 8, 8), np.float32)
        self._ck(self.lib.pmp_infer_q(self.h, COMP_ID[comp], int(qp), _ptr(by), _ptr(bu), _ptr(bv), n, _ptr(qt)))
        return qt

    def post_process(self, qt, bt, dire, comp):
        """eli_structual_error + Map_to_Partition per block (Metrics.py:764-774 without the file).
        qt RAW logits f32[N,(1,)8,8]; returns hor, ver u8[N,16,16], qt_u8 u8[N,8,8], dire_i8 i8[N,3,16,16]."""
        qt = np.ascontiguousarray(qt, np.float32); bt = np.ascontiguousarray(bt, np.float32); dire = np.ascontiguousarray(dire, np.float32)
        n = qt.size // 64
        if qt.size != n * 64 or bt.size != n * 768 or dire.size != n * 768:
            raise ValueError("post_process: expected qt[N,8,8], bt[N,3,16,16], dire[N,3,16,16]")
        hor = np.empty((n, 16, 16), np.uint8); ver = np.empty((n, 16, 16), np.uint8)
        q8 = np.empty((n, 8, 8), np.uint8); d8 = np.empty((n, 3, 16, 16), np.int8)
        self._ck(self.lib.pmp_postprocess(self.h, COMP_ID[comp], _ptr(qt), _ptr(bt), _ptr(dire), n, _ptr(hor), _ptr(ver), _ptr(q8), _ptr(d8)))
        return hor, ver, q8, d8

    def seq_post_process(self, input_qt_batch, input_bt_batch, input_dire_batch, comp, sub_numfrm, width, height, save_path,
                         lamb1=None, lamb2=None, lamb3=None, lamb4=None, lamb5=None, thd=None):
        """Metrics.py:764-774: post-process every block of a sequence and write the PartitionMat file.  lamb1..lamb5 / thd (optional):
        Map_to_Partition's thresholds for this call only (see set_partition_params); the component's set is restored afterwards."""
        n_expected = int(sub_numfrm) * (int(height) // 64) * (int(width) // 64)
        kw = {k: v for k, v in zip(PARAM_KEYS, (lamb1, lamb2, lamb3, lamb4, lamb5, thd)) if v is not None}
        if kw:
            old = self._params(comp)
            self.set_partition_params(comp, **kw)
            try:
                hor, ver, q8, d8 = self.post_process(input_qt_batch, input_bt_batch, input_dire_batch, comp)
            finally:
                self._ck(self.lib.pmp_set_partition_params(self.h, COMP_ID[comp], C.byref(old)))
        else:
            hor, ver, q8, d8 = self.post_process(input_qt_batch, input_bt_batch, input_dire_batch, comp)
        if hor.shape[0] != n_expected:
            raise ValueError("seq_post_process: %d blocks given, geometry needs %d" % (hor.shape[0], n_expected))
        if save_path is not None:
            write_partition_file(save_path, sub_numfrm, height, width, hor, ver, q8, d8)
        return hor, ver, q8, d8

    def infer_postprocess(self, comp, qp, block_y, block_u=None, block_v=None, want_logits=False):
        by, bu, bv = _u8(block_y), _u8(block_u), _u8(block_v)
        n = self._check_blocks(comp, by, bu, bv)
        self.load(comp, qp)
        hor = np.empty((n, 16, 16), np.uint8); ver = np.empty((n, 16, 16), np.uint8)
        q8 = np.empty((n, 8, 8), np.uint8); d8 = np.empty((n, 3, 16, 16), np.int8)
        qt = bt = dire = None
        if want_logits:
            qt = np.empty((n, 1, 8, 8), np.float32); bt = np.empty((n, 3, 16, 16), np.float32); dire = np.empty((n, 3, 16, 16), np.float32)
        self._ck(self.lib.pmp_infer_postprocess(self.h, COMP_ID[comp], int(qp), _ptr(by), _ptr(bu), _ptr(bv), n, _ptr(hor), _ptr(ver),
                                                _ptr(q8), _ptr(d8), _ptr(qt), _ptr(bt), _ptr(dire)))
        return (hor, ver, q8, d8, qt, bt, dire) if want_logits else (hor, ver, q8, d8)

    def output_block_yuv(self, y, u, v, bitdepth=8):
        """Inference_QBD.py:104-149 on already-loaded planes y[F,H,W], u,v[F,H/2,W/2] (u8, or u16 for 10-bit)."""
        dt = np.uint8 if bitdepth == 8 else np.uint16
        y = np.ascontiguousarray(y, dt); u = np.ascontiguousarray(u, dt); v = np.ascontiguousarray(v, dt)
        F, H, Wd = y.shape
        if u.shape != (F, H // 2, Wd // 2) or v.shape != u.shape:
            raise ValueError("output_block_yuv: chroma planes must be [F, H/2, W/2]")
        n = F * (H // 64) * (Wd // 64)
        by = np.empty((n, 68, 68), np.uint8); bu = np.empty((n, 34, 34), np.uint8); bv = np.empty((n, 34, 34), np.uint8)
        self._ck(self.lib.pmp_cut_blocks(self.h, _ptr(y), _ptr(u), _ptr(v), F, H, Wd, int(bitdepth), _ptr(by), _ptr(bu), _ptr(bv)))
        return by, bu, bv

    # ------------------------------------------------------------------------------------------ training labels
    def gen_seq_sub_map(self, qt_map, bt_map, dire_map, is_luma, return_status=False):
        """GenMSBtMap.gen_seq_sub_map (GenMSBtMap.py:434-449): qt_map [N,8,8] (qtDepth - 1), bt_map [N,16,16], dire_map [N,3,16,16]
        -> msbt u8[N,3,16,16] (and status u8[N], include/pmp.h: pmp_msbt_labels, with return_status).  is_luma picks the chroma factor
        as the reference does (1, else 2).  Values must fit the reference's dtypes (u8, u8, i8): anything else is refused, not wrapped."""
        qt = _fit(qt_map, np.uint8, "qt_map"); bt = _fit(bt_map, np.uint8, "bt_map"); dire = _fit(dire_map, np.int8, "dire_map")
        n = qt.size // 64
        if qt.size != n * 64 or bt.size != n * 256 or dire.size != n * 768:
            raise ValueError("gen_seq_sub_map: expected qt_map[N,8,8], bt_map[N,16,16], dire_map[N,3,16,16]")
        msbt = np.empty((n, 3, 16, 16), np.uint8); st = np.empty(n, np.uint8)
        self._ck(self.lib.pmp_msbt_labels(self.h, 1 if is_luma else 2, _ptr(qt), _ptr(bt), _ptr(dire), n, _ptr(msbt), _ptr(st)))
        return (msbt, st) if return_status else msbt

    def getSubMap(self, qt_map, bt_map, dire_map, chroma_factor, return_status=False):
        """GenMSBtMap.getSubMap (:370-375) for one block: qt_map [8,8], bt_map [16,16], dire_map [3,16,16] -> u8[3,16,16]."""
        if chroma_factor not in (1, 2):
            raise ValueError("getSubMap: chroma_factor must be 1 or 2")
        m, st = self.gen_seq_sub_map(np.reshape(qt_map, (1, 8, 8)), np.reshape(bt_map, (1, 16, 16)), np.reshape(dire_map, (1, 3, 16, 16)),
                                     chroma_factor == 1, return_status=True)
        return (m[0], int(st[0])) if return_status else m[0]

    def msbt_labels_device(self, cf, d_qt, d_bt, d_dire, n, d_msbt, d_status):
        """pmp_msbt_labels_device: device pointers (u8 qt, u8 bt, i8 dire in; u8 msbt, u8 status out), stream-ordered."""
        self._ck(self.lib.pmp_msbt_labels_device(self.h, int(cf), d_qt, d_bt, d_dire, int(n), d_msbt, d_status))

    # ------------------------------------------------------------------------------------------ the labels' own partition
    def label_partition(self, qt_map, bt_map, dire_map, cf):
        """GenMSBtMap.map_to_parititon (GenMSBtMap.py:377-382) on every block: qt_map [N,8,8] (qtDepth - 1), bt_map [N,16,16], dire_map
        [N,3,16,16], chroma factor cf (1 or 2) -> hor, ver u8[N,16,16], status u8[N] (include/pmp.h: pmp_label_partition).  Values must
        fit the reference's dtypes (u8, u8, i8): anything else is refused, not wrapped."""
        if cf not in (1, 2):
            raise ValueError("label_partition: cf must be 1 or 2")
        qt = _fit(qt_map, np.uint8, "qt_map"); bt = _fit(bt_map, np.uint8, "bt_map"); dire = _fit(dire_map, np.int8, "dire_map")
        n = qt.size // 64
        if qt.size != n * 64 or bt.size != n * 256 or dire.size != n * 768:
            raise ValueError("label_partition: expected qt_map[N,8,8], bt_map[N,16,16], dire_map[N,3,16,16]")
        hor = np.empty((n, 16, 16), np.uint8); ver = np.empty((n, 16, 16), np.uint8); st = np.empty(n, np.uint8)
        self._ck(self.lib.pmp_label_partition(self.h, int(cf), _ptr(qt), _ptr(bt), _ptr(dire), n, _ptr(hor), _ptr(ver), _ptr(st)))
        return hor, ver, st

    def label_partition_for_VTM(self, qt_map, bt_map, dire_map, is_luma, save_path, frm_num, frm_width, frm_height, binary=False):
        """GenMSBtMap.get_sequence_partition_for_VTM (GenMSBtMap.py:384-432) without its plot: the labels of one sequence (blocks
        frame-major, row-major; qt_map is qtDepth - 1) -> the PartitionMat file of a perfect predictor at save_path (None: no file).
        Chroma factor 1 for luma, 2 otherwise, as there.  The file's qt and direction sections are the labels themselves (:407-408);
        the text is what write_partition_file writes, so a direction of -1 is printed as -1 where the reference prints 255
        (include/pmp.h: pmp_label_partition); binary=True writes the PMPB1 side channel instead.  Returns hor, ver, status."""
        n_expected = int(frm_num) * (int(frm_height) // 64) * (int(frm_width) // 64)
        hor, ver, st = self.label_partition(qt_map, bt_map, dire_map, 1 if is_luma else 2)
        if hor.shape[0] != n_expected:
            raise ValueError("label_partition_for_VTM: %d blocks given, geometry needs %d" % (hor.shape[0], n_expected))
        if save_path is not None:
            write = write_partition_binary if binary else write_partition_file
            write(save_path, frm_num, frm_height, frm_width, hor, ver, _fit(qt_map, np.uint8, "qt_map"), _fit(dire_map, np.int8, "dire_map"))
        return hor, ver, st

    def label_partition_device(self, cf, d_qt, d_bt, d_dire, n, d_hor, d_ver, d_status):
        """pmp_label_partition_device: device pointers (u8 qt, u8 bt, i8 dire in; u8 hor, u8 ver, u8 status out), stream-ordered."""
        self._ck(self.lib.pmp_label_partition_device(self.h, int(cf), d_qt, d_bt, d_dire, int(n), d_hor, d_ver, d_status))

    def label_partition_records_device(self, cf, d_qt, d_bt, d_dire, n, d_rec, d_status):
        """pmp_label_partition_records_device: one packed 1344-byte record per block (hor | ver | qt | dire) and u8 status."""
        self._ck(self.lib.pmp_label_partition_records_device(self.h, int(cf), d_qt, d_bt, d_dire, int(n), d_rec, d_status))

    # ------------------------------------------------------------------------------------------ validation
    def val_stats(self, qp, qt=None, bt=None, dire=None, qt8=None, msbt=None, msdire=None):
        """pmp_val_stats (include/pmp.h): the twenty per-batch numbers S[0..19] of logits against labels, the whole call as one batch.
        qt f32[N,(1,)8,8] with qt8 u8[N,8,8] (RAW qtDepth), bt / dire f32[N,3,16,16] with msbt u8 / msdire i8 [N,3,16,16]; leave the
        QT pair or the MTT four out for the MTT-only / QT-only forms.  -> float64[20]."""
        (qt, bt, dire, qt8, msbt, msdire), n = _logit_label_arrays(qt, bt, dire, qt8, msbt, msdire)
        out = np.zeros(_lib.PMP_VAL_NSTATS, np.float64)
        self._ck(self.lib.pmp_val_stats(self.h, int(qp), _ptr(qt), _ptr(bt), _ptr(dire), _ptr(qt8), _ptr(msbt), _ptr(msdire), n, _ptr(out)))
        return out

    def val_stats_device(self, qp, d_qt, d_bt, d_dire, d_qt8, d_msbt, d_msdire, n, d_stats, d_block_stats=None):
        """pmp_val_stats_device: device pointers (None for the pair / the four left out), f64[20] -> d_stats and, if given, the per-block
        partials f64[n,20] -> d_block_stats; stream-ordered, final after synchronize() (include/pmp.h: range guard)."""
        self._ck(self.lib.pmp_val_stats_device(self.h, int(qp), d_qt, d_bt, d_dire, d_qt8, d_msbt, d_msdire, int(n), d_stats, d_block_stats))

    def val_confusion(self, qt=None, bt=None, dire=None, qt8=None, msbt=None, msdire=None):
        """pmp_val_confusion (include/pmp.h): per map (qt, bt0..2, dire0..2) the joint histogram of (label class, predicted class), the
        whole call as one batch.  Arrays as val_stats takes them; a group's labels without its logits give the labels' census.
        -> int64[7,5,5]."""
        a, n = _logit_label_arrays(qt, bt, dire, qt8, msbt, msdire, census=True)
        out = np.zeros((_lib.PMP_CONF_MAPS, _lib.PMP_CONF_CLASSES, _lib.PMP_CONF_CLASSES), np.int64)
        self._ck(self.lib.pmp_val_confusion(self.h, *[_ptr(x) for x in a], n, _ptr(out)))
        return out

    def val_confusion_device(self, d_qt, d_bt, d_dire, d_qt8, d_msbt, d_msdire, n, d_counts, d_block_counts=None):
        """pmp_val_confusion_device: device pointers (None for what is left out), i64[175] -> d_counts and, if given, the per-block counts
        u16[n,175] -> d_block_counts; stream-ordered, final after synchronize() (include/pmp.h: range guard)."""
        self._ck(self.lib.pmp_val_confusion_device(self.h, d_qt, d_bt, d_dire, d_qt8, d_msbt, d_msdire, int(n), d_counts, d_block_counts))

    confusion_summary = staticmethod(confusion_summary)     # validation.confusion_summary(C): what the counts say, per map

    # ------------------------------------------------------------------------------------------ training losses
    def train_loss(self, comp, qp, qt=None, bt=None, dire=None, qt8=None, msbt=None, msdire=None, params=None, want_grads=True):
        """pmp_train_loss (include/pmp.h): Train_QBD.loss_func_QBD (all six given), loss_func_MSBD (no qt, qt8) or pre_train_Q's L1 (qt, qt8
        only) of one batch, and the gradient of that loss with respect to the logits.  Arrays as val_stats takes them; params: a dict with
        any of LOSS_KEYS, a "lambb0=0.8,..." text or a LossParams (None: Train_QBD's defaults).
        -> (terms float64[13], loss float, grads): grads is None without want_grads, else {"qt": f32[N,8,8], "bt": f32[N,3,16,16],
        "dire": f32[N,3,16,16]} with the entries of the logits given."""
        (qt, bt, dire, qt8, msbt, msdire), n = _logit_label_arrays(qt, bt, dire, qt8, msbt, msdire)
        terms = np.zeros(_lib.PMP_LOSS_NTERMS, np.float64)
        loss = np.zeros(1, np.float64)
        grads = None
        if want_grads:
            grads = {}
            if qt is not None:
                grads["qt"] = np.empty((n, 8, 8), np.float32)
            if bt is not None:
                grads["bt"] = np.empty((n, 3, 16, 16), np.float32); grads["dire"] = np.empty((n, 3, 16, 16), np.float32)
        g = grads or {}
        self._ck(self.lib.pmp_train_loss(self.h, COMP_ID[comp], int(qp), loss_params(params), _ptr(qt), _ptr(bt), _ptr(dire), _ptr(qt8), _ptr(msbt),
                                         _ptr(msdire), n, _ptr(terms), _ptr(loss), _ptr(g.get("qt")), _ptr(g.get("bt")), _ptr(g.get("dire"))))
        return terms, float(loss[0]), grads

    def train_loss_device(self, comp, qp, d_qt, d_bt, d_dire, d_qt8, d_msbt, d_msdire, n, d_terms, d_loss, d_g_qt=None, d_g_bt=None,
                          d_g_dire=None, params=None):
        """pmp_train_loss_device: device pointers (None for the pair / the four left out; gradients all None or those of the logits given),
        f64[13] -> d_terms, f64 -> d_loss; stream-ordered on the engine's stream, the host does not wait."""
        self._ck(self.lib.pmp_train_loss_device(self.h, COMP_ID[comp], int(qp), loss_params(params), d_qt, d_bt, d_dire, d_qt8, d_msbt, d_msdire,
                                                int(n), d_terms, d_loss, d_g_qt, d_g_bt, d_g_dire))

    # ------------------------------------------------------------------------------------------ one ResidualBlock, forward and backward
    @staticmethod
    def _rb_arrays(**arrays):
        """float32 C-contiguous copies of the arrays of one ResidualBlock call and its RbShape, derived from x and w0; every other array
        given must have exactly the shape that follows (the C call reads that many floats)."""
        a = {k: None if v is None else np.ascontiguousarray(v, np.float32) for k, v in arrays.items()}
        if a["x"].ndim != 4 or a["w0"].ndim != 4:
            raise ValueError("resblock: x must be [n, cin, h, w] and w0 [cout, cin, k, k]")
        n, cin, h, w = a["x"].shape
        cout, cin_w, k, k2 = a["w0"].shape
        if cin_w != cin or k != k2:
            raise ValueError("resblock: w0 must be [cout, cin, k, k] for x [n, cin, h, w]")
        want = {"w2": [(cout, cout, k, k)], "wsc": [(cout, cin), (cout, cin, 1, 1)], "t": [(n, cout, h, w)], "out": [(n, cout, h, w)],
                "g_out": [(n, cout, h, w)]}
        for key, v in a.items():
            if key in want and v is not None and v.shape not in want[key]:
                raise ValueError("resblock: %s has shape %s, expected %s" % (key, v.shape, want[key][0]))
        if (a.get("wsc") is not None) != (cin != cout):
            raise ValueError("resblock: wsc is passed exactly when cin != cout")
        return a, _lib.RbShape(n, h, w, cin, cout, k)

    def resblock_forward(self, x, w0, w2, wsc=None):
        """pmp_resblock_forward (include/pmp.h): Model_QBD.ResidualBlock on the fp32 MFMA datapath.  x f32[n,cin,h,w], w0 [cout,cin,k,k],
        w2 [cout,cout,k,k], wsc [cout,cin(,1,1)] exactly when cin != cout.  -> (t, out) f32[n,cout,h,w]: the activation between the two
        convolutions, which the backward pass needs, and the block's output."""
        a, s = self._rb_arrays(x=x, w0=w0, w2=w2, wsc=wsc)
        t = np.empty((s.n, s.cout, s.h, s.w), np.float32); out = np.empty_like(t)
        self._ck(self.lib.pmp_resblock_forward(self.h, C.byref(s), _ptr(a["x"]), _ptr(a["w0"]), _ptr(a["w2"]), _ptr(a["wsc"]), _ptr(t), _ptr(out)))
        return t, out

    def resblock_backward(self, x, t, out, w0, w2, wsc, g_out, want_g_x=True):
        """pmp_resblock_backward: the gradients of the block from its saved x, t, out and the upstream gradient g_out f32[n,cout,h,w].
        -> (g_x or None without want_g_x, g_w0, g_w2, g_wsc or None for an identity shortcut), shaped like x, w0, w2, wsc."""
        a, s = self._rb_arrays(x=x, t=t, out=out, w0=w0, w2=w2, wsc=wsc, g_out=g_out)
        g_x = np.empty_like(a["x"]) if want_g_x else None
        g_w0, g_w2 = np.empty_like(a["w0"]), np.empty_like(a["w2"])
        g_wsc = None if a["wsc"] is None else np.empty_like(a["wsc"])
        self._ck(self.lib.pmp_resblock_backward(self.h, C.byref(s), *[_ptr(a[k]) for k in ("x", "t", "out", "w0", "w2", "wsc", "g_out")],
                                                _ptr(g_x), _ptr(g_w0), _ptr(g_w2), _ptr(g_wsc)))
        return g_x, g_w0, g_w2, g_wsc

    def resblock_forward_device(self, shape, d_x, d_w0, d_w2, d_wsc, d_t, d_out):
        """pmp_resblock_forward_device: shape = (n, h, w, cin, cout, k), device pointers (d_wsc None for an identity shortcut);
        stream-ordered on the engine's stream, the host does not wait."""
        s = _lib.RbShape(*(int(v) for v in shape))
        self._ck(self.lib.pmp_resblock_forward_device(self.h, C.byref(s), d_x, d_w0, d_w2, d_wsc, d_t, d_out))

    def resblock_backward_device(self, shape, d_x, d_t, d_out, d_w0, d_w2, d_wsc, d_g_out, d_g_x, d_g_w0, d_g_w2, d_g_wsc):
        """pmp_resblock_backward_device: as above; d_g_x None = not computed, d_wsc and d_g_wsc None for an identity shortcut."""
        s = _lib.RbShape(*(int(v) for v in shape))
        self._ck(self.lib.pmp_resblock_backward_device(self.h, C.byref(s), d_x, d_t, d_out, d_w0, d_w2, d_wsc, d_g_out, d_g_x, d_g_w0, d_g_w2,
                                                       d_g_wsc))

    # ------------------------------------------------------------------------------------------ a trunk of ResidualBlocks, kept blocked
    @staticmethod
    def _saved_bytes(name, struct, shape):
        size = getattr(_lib.load(), name)(C.byref(struct(shape)))
        if size < 0:                                   # no context, so no pmp_last_error
            raise _lib.PmpError(int(size), "%s: unsupported shape %s" % (name, tuple(shape)))
        return size

    @staticmethod
    def trunk_saved_bytes(shape):
        """pmp_trunk_saved_bytes: the size of the saved-activation buffer of shape = (n, h, w, cin, [(cout, k), ...], pool)."""
        return Engine._saved_bytes("pmp_trunk_saved_bytes", _lib.trunk_shape, shape)

    def trunk_forward_device(self, shape, d_x, d_w, d_saved, d_y):
        """pmp_trunk_forward_device: d_w = 3 device pointers per block (w0, w2, wsc or None); d_saved trunk_saved_bytes(shape) bytes,
        16-byte aligned; stream-ordered on the engine's stream, the host does not wait."""
        s = _lib.trunk_shape(shape)
        self._ck(self.lib.pmp_trunk_forward_device(self.h, C.byref(s), d_x, _lib.pointer_array(d_w, 3 * s.nblocks), d_saved, d_y))

    def trunk_backward_device(self, shape, d_saved, d_w, d_g_y, d_g_x, d_g_w):
        """pmp_trunk_backward_device: d_g_x None = not computed; d_g_w None exactly where d_w is."""
        s = _lib.trunk_shape(shape)
        self._ck(self.lib.pmp_trunk_backward_device(self.h, C.byref(s), d_saved, _lib.pointer_array(d_w, 3 * s.nblocks), d_g_y, d_g_x,
                                                    _lib.pointer_array(d_g_w, 3 * s.nblocks)))

    def trunk_unpack_device(self, shape, d_saved, index, d_dense):
        """pmp_trunk_unpack_device: saved tensor `index` (0: x; 2i + 1: t_i; 2i + 2: out_i, un-pooled) -> torch's dense layout."""
        s = _lib.trunk_shape(shape)
        self._ck(self.lib.pmp_trunk_unpack_device(self.h, C.byref(s), d_saved, int(index), d_dense))

    # ------------------------------------------------------------------------------------------ a QT net's tail: resblock_q3 .. q6
    @staticmethod
    def qtail_saved_bytes(shape):
        """pmp_qtail_saved_bytes: the size of the saved-activation buffer of shape = (n, h, w), the map of x4."""
        return Engine._saved_bytes("pmp_qtail_saved_bytes", _lib.qtail_shape, shape)

    def qtail_forward_device(self, shape, d_x4, d_w, d_saved, d_x9):
        """pmp_qtail_forward_device: d_w = 12 device pointers, w0, w2, wsc of q3, q4, q5 (wsc None), q6; d_saved
        qtail_saved_bytes(shape) bytes, 16-byte aligned; stream-ordered on the engine's stream, the host does not wait."""
        self._ck(self.lib.pmp_qtail_forward_device(self.h, C.byref(_lib.qtail_shape(shape)), d_x4, _lib.pointer_array(d_w, 12), d_saved, d_x9))

    def qtail_backward_device(self, shape, d_saved, d_w, d_g_x9, d_g_x4, d_g_w):
        """pmp_qtail_backward_device: d_g_x4 None = not computed; d_g_w None exactly where d_w is."""
        self._ck(self.lib.pmp_qtail_backward_device(self.h, C.byref(_lib.qtail_shape(shape)), d_saved, _lib.pointer_array(d_w, 12), d_g_x9,
                                                    d_g_x4, _lib.pointer_array(d_g_w, 12)))

    def qtail_unpack_device(self, shape, d_saved, index, d_dense):
        """pmp_qtail_unpack_device: saved tensor `index` (0: x4; 1, 2: t, out of q3; 3, 4: q4; 5, 6: q5, un-pooled; 7, 8: q6 at half
        resolution) -> torch's dense layout."""
        self._ck(self.lib.pmp_qtail_unpack_device(self.h, C.byref(_lib.qtail_shape(shape)), d_saved, int(index), d_dense))

    # ------------------------------------------------------------------------------------------ a net's stem, forward and backward
    @staticmethod
    def _stem_arrays(*arrays):
        """d_w, d_b, ...: one pointer or a sequence of one (split 0) or three -> host arrays of three pointers, the missing ones NULL."""
        out = []
        for a in arrays:
            a = list(a) if isinstance(a, (list, tuple)) else [a]
            out.append(_lib.pointer_array(a + [None] * (3 - len(a)), 3))
        return out

    def stem_forward_device(self, shape, d_x, d_w, d_b, d_y):
        """pmp_stem_forward_device: shape = (n, h, w, cin, k, split); d_w and d_b one device pointer (split 0) or three (split 1);
        stream-ordered on the engine's stream, the host does not wait."""
        s = _lib.stem_shape(shape)
        w, b = self._stem_arrays(d_w, d_b)
        self._ck(self.lib.pmp_stem_forward_device(self.h, C.byref(s), d_x, w, b, d_y))

    def stem_backward_device(self, shape, d_x, d_y, d_w, d_g_y, d_g_x, d_g_w, d_g_b):
        """pmp_stem_backward_device: as above; d_g_x None = not computed."""
        s = _lib.stem_shape(shape)
        w, g_w, g_b = self._stem_arrays(d_w, d_g_w, d_g_b)
        self._ck(self.lib.pmp_stem_backward_device(self.h, C.byref(s), d_x, d_y, w, d_g_y, d_g_x, g_w, g_b))

    # ------------------------------------------------------------------------------------------ an MTT net's heads and gate products
    def head_forward_device(self, shape, d_x, d_w, d_b, d_prev, d_q, d_y, d_att):
        """pmp_head_forward_device: shape = (n, h, w, cin, cout, up_q, up_y); d_prev None = no carry; d_q and d_att exactly when
        up_y != 0; stream-ordered on the engine's stream, the host does not wait."""
        self._ck(self.lib.pmp_head_forward_device(self.h, C.byref(_lib.head_shape(shape)), d_x, d_w, d_b, d_prev, d_q, d_y, d_att))

    def head_backward_device(self, shape, d_x, d_w, d_g_y, d_g_att, d_g_x, d_g_w, d_g_b, d_g_q=None, d_g_prev=None):
        """pmp_head_backward_device: d_g_att exactly when up_y != 0; d_g_x, d_g_q, d_g_prev None = not computed."""
        self._ck(self.lib.pmp_head_backward_device(self.h, C.byref(_lib.head_shape(shape)), d_x, d_w, d_g_y, d_g_att, d_g_x, d_g_w, d_g_b,
                                                   d_g_q, d_g_prev))

    def gate_forward_device(self, count, d_x, d_a, d_y):
        """pmp_gate_forward_device: y = x * a over count floats."""
        self._ck(self.lib.pmp_gate_forward_device(self.h, int(count), d_x, d_a, d_y))

    def gate_backward_device(self, count, d_x, d_a, d_g_y, d_g_acc, d_g_x, d_g_a):
        """pmp_gate_backward_device: g_a = g_y * x, g_x = g_y * a, or d_g_acc + g_y * a when d_g_acc is given."""
        self._ck(self.lib.pmp_gate_backward_device(self.h, int(count), d_x, d_a, d_g_y, d_g_acc, d_g_x, d_g_a))

    # ------------------------------------------------------------------------------------------ a training step's ends
    def batch_gather_device(self, src, d_index, n, d_status, d_x=None, d_qt_f=None, d_qt8=None, d_msbt=None, d_msdire=None):
        """pmp_batch_gather_device: src a _lib.BatchSrc (the whole set on the device), d_index i64[n], the outputs asked for (None: not),
        d_status an int32 word the caller zeroed; stream-ordered on the engine's stream, the host does not wait."""
        dst = _lib.BatchDst(d_x, d_qt_f, d_qt8, d_msbt, d_msdire)
        self._ck(self.lib.pmp_batch_gather_device(self.h, C.byref(src), d_index, int(n), C.byref(dst), d_status))

    def adam_step_device(self, d_param, d_grad, d_m, d_v, counts, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        """pmp_adam_step_device: lists of device pointers and of element counts, one entry per tensor; step >= 1 is the step this call
        performs (torch.optim.Adam, no weight decay, no amsgrad); one launch, stream-ordered, the host does not wait."""
        nt = len(counts)
        p = _lib.AdamParams(float(lr), float(betas[0]), float(betas[1]), float(eps))
        self._ck(self.lib.pmp_adam_step_device(self.h, C.byref(p), nt, _lib.pointer_array(d_param, nt), _lib.pointer_array(d_grad, nt),
                                               _lib.pointer_array(d_m, nt), _lib.pointer_array(d_v, nt), (C.c_int64 * nt)(*[int(k) for k in counts]),
                                               int(step)))

    def grad_guard_scratch_bytes(self, counts):
        """pmp_grad_guard_scratch_bytes: the bytes of grad_guard_device's d_scratch for tensors of counts[i] floats (host only)."""
        nt = len(counts)
        n = int(self.lib.pmp_grad_guard_scratch_bytes(nt, (C.c_int64 * nt)(*[int(k) for k in counts])))
        if n < 0:
            raise ValueError("grad_guard_scratch_bytes: at least one tensor, every count in 1 .. 2^30 - 1")
        return n

    def grad_guard_device(self, d_grad, counts, d_scratch, d_record, d_state=None, max_norm=0.0, skip_nonfinite=False):
        """pmp_grad_guard_device: the global norm and non-finite census of the gradients (device pointers, counts[i] floats each), in an
        order fixed by the counts, into the 32-byte record at d_record (_lib.GuardRecord) and, where given, the running counters at
        d_state (_lib.GuardState, zeroed once by the caller); two launches up to 96 tensors, stream-ordered, the host does not wait."""
        nt = len(counts)
        p = _lib.GuardParams(float(max_norm), 1 if skip_nonfinite else 0)
        self._ck(self.lib.pmp_grad_guard_device(self.h, C.byref(p), nt, _lib.pointer_array(d_grad, nt), (C.c_int64 * nt)(*[int(k) for k in counts]),
                                                d_scratch, d_record, d_state))

    def adam_step_guarded_device(self, d_param, d_grad, d_m, d_v, counts, step, d_record, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        """pmp_adam_step_guarded_device: adam_step_device taking its orders from grad_guard_device's record in device memory: nothing
        is written with the skip bit set, else the gradients count times the record's coef.  A skipped step still counts as a step."""
        nt = len(counts)
        p = _lib.AdamParams(float(lr), float(betas[0]), float(betas[1]), float(eps))
        self._ck(self.lib.pmp_adam_step_guarded_device(self.h, C.byref(p), nt, _lib.pointer_array(d_param, nt), _lib.pointer_array(d_grad, nt),
                                                       _lib.pointer_array(d_m, nt), _lib.pointer_array(d_v, nt),
                                                       (C.c_int64 * nt)(*[int(k) for k in counts]), int(step), d_record))

    def grad_pack_device(self, d_grad, counts, d_bucket):
        """pmp_grad_pack_device: the gradients (device pointers, None = a parameter without one: zeros) of counts[i] floats each into
        the bucket grad_bucket_floats(counts) lays out; every float of the bucket is written; stream-ordered, the host does not wait."""
        nt = len(counts)
        self._ck(self.lib.pmp_grad_pack_device(self.h, nt, _lib.pointer_array(d_grad, nt), (C.c_int64 * nt)(*[int(k) for k in counts]), d_bucket))

    def grad_sum_device(self, d_src, count, d_dst):
        """pmp_grad_sum_device: d_dst = ((d_src[0] + d_src[1]) + ...) over count floats, float32 additions in the list's order; d_dst
        may be d_src[0]; stream-ordered, the host does not wait."""
        d_src = list(d_src)
        self._ck(self.lib.pmp_grad_sum_device(self.h, len(d_src), _lib.pointer_array(d_src, len(d_src)) if d_src else None, int(count), d_dst))

    # ------------------------------------------------------------------------------------------ data set assembly
    def select_rows_device(self, d_flags, mask, d_seg_end, nseg, cap, n, d_index, d_count):
        """pmp_select_rows_device: d_flags a list of device pointers to u8[n] (empty: every row is a candidate), d_seg_end i64[nseg],
        d_index i64[n] and d_count i64[nseg + 1] out; stream-ordered on the engine's stream, the host does not wait."""
        d_flags = list(d_flags or ())
        self._ck(self.lib.pmp_select_rows_device(self.h, _lib.pointer_array(d_flags, len(d_flags)) if d_flags else None, len(d_flags), int(mask),
                                                 d_seg_end, int(nseg), int(cap), int(n), d_index, d_count))

    def gather_rows_device(self, d_src, nsrc, row_bytes, d_index, m, d_dst, d_status):
        """pmp_gather_rows_device: row j of d_dst = row d_index[j] of d_src, row_bytes bytes each; d_status an int32 word the caller
        zeroed (bit 0: an index outside the source, its row zeros); stream-ordered, the host does not wait."""
        self._ck(self.lib.pmp_gather_rows_device(self.h, d_src, int(nsrc), int(row_bytes), d_index, int(m), d_dst, d_status))

    def select_rows(self, flags, mask, seg_end, cap=0, n=None):
        """The host form of select_rows_device: flags a list of u8[n] arrays (empty: give n), seg_end the segments' ends (ascending,
        the last one n) -> (index i64[m], the kept rows in ascending order; counts i64[nseg + 1], per segment and, last, m)."""
        import torch
        flags = [np.ascontiguousarray(f, np.uint8).reshape(-1) for f in flags]
        seg_end = np.ascontiguousarray(seg_end, np.int64).reshape(-1)
        n = int(n) if n is not None else (flags[0].size if flags else int(seg_end[-1]))
        if any(f.size != n for f in flags):
            raise ValueError("select_rows: every flag array must have n = %d entries" % n)
        dev = torch.device("cuda", int(self.device))
        d_flags = [torch.from_numpy(f).to(dev) for f in flags]
        d_seg = torch.from_numpy(seg_end).to(dev)
        d_index = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        d_count = torch.empty(seg_end.size + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)                       # the uploads ran on torch's stream; the context has its own
        self.select_rows_device([t.data_ptr() for t in d_flags], mask, d_seg.data_ptr(), seg_end.size, cap, n, d_index.data_ptr(), d_count.data_ptr())
        self.synchronize()
        counts = d_count.cpu().numpy()
        return d_index[:int(counts[-1])].cpu().numpy(), counts

    def gather_rows(self, src, index):
        """The host form of gather_rows_device: src[index] along the first axis (rows of a multiple of 4 bytes, at most 65536); an
        index outside the array raises IndexError."""
        import torch
        src = np.ascontiguousarray(src)
        index = np.ascontiguousarray(index, np.int64).reshape(-1)
        row_bytes = src[0].nbytes if len(src) else 0
        out = np.empty((index.size,) + src.shape[1:], src.dtype)
        if index.size == 0:
            return out
        dev = torch.device("cuda", int(self.device))
        d_src = torch.from_numpy(src.view(np.uint8).reshape(len(src), -1)).to(dev)
        d_index = torch.from_numpy(index).to(dev)
        d_dst = torch.empty((index.size, row_bytes), dtype=torch.uint8, device=dev)
        d_status = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.gather_rows_device(d_src.data_ptr(), len(src), row_bytes, d_index.data_ptr(), index.size, d_dst.data_ptr(), d_status.data_ptr())
        self.synchronize()
        if int(d_status.item()):
            raise IndexError("gather_rows: an index lies outside the %d rows of the array" % len(src))
        out.view(np.uint8).reshape(index.size, -1)[:] = d_dst.cpu().numpy()
        return out

    def infer_msbd(self, comp, qp, qt_in, block_y, block_u=None, block_v=None):
        """Teacher-forced MTT inference (pmp_infer_msbd; Net(input_batch, qt_label_batch), Metrics.py:226): the MTT net of (comp, qp) on
        the blocks with the GIVEN QT map qt_in f32[N,(1,)8,8] -> bt f32[N,3,16,16], dire f32[N,3,16,16]."""
        by, bu, bv = _u8(block_y), _u8(block_u), _u8(block_v)
        n = self._check_blocks(comp, by, bu, bv)
        q = np.ascontiguousarray(qt_in, np.float32)
        if q.size != n * 64:
            raise ValueError("infer_msbd: qt_in must be f32[N,8,8] for the N blocks given")
        self.load(comp, qp)
        bt = np.empty((n, 3, 16, 16), np.float32); dire = np.empty((n, 3, 16, 16), np.float32)
        self._ck(self.lib.pmp_infer_msbd(self.h, COMP_ID[comp], int(qp), _ptr(by), _ptr(bu), _ptr(bv), _ptr(q), n, _ptr(bt), _ptr(dire)))
        return bt, dire

    def infer_msbd_device(self, comp, qp, d_by, d_bu, d_bv, d_qt_in, n, d_bt, d_dire):
        self._ck(self.lib.pmp_infer_msbd_device(self.h, COMP_ID[comp], int(qp), d_by, d_bu, d_bv, d_qt_in, int(n), d_bt, d_dire))

    def validation_QBD(self, comp, qp, blocks, qt8, msbt, msdire, batch_size=200, logits=None, return_block_stats=False, batch_range=None,
                       return_confusion=False):
        """Metrics.validation_QBD (Metrics.py:313-385) on the GPU: both nets on every batch, the QT net's output feeding the MTT net.
        blocks: block_y u8[N,68,68] (Luma) or (block_y, block_u, block_v) (Chroma); labels as the label files hold them (qt8 RAW
        qtDepth u8[N,8,8], msbt u8 / msdire i8 [N,3,16,16]).  The set is cut into batches of batch_size IN ORDER (the reference
        shuffles: its numbers are defined up to that; the ragged last batch weighs like a full one, as there).  Returns the
        reference's list of 15: [q_L1, b0_L1, b1_L1, b2_L1, d0_L1, d1_L1, d2_L1, q_accu, b0_accu, b1_accu, b2_accu, d0_accu, d1_accu,
        d2_accu, val_loss], each np.mean over the per-batch values.  logits = (qt, bt, dire): validate these instead of running the
        nets (blocks may be None).  return_block_stats: also the per-block partials float64[N,20] (include/pmp.h: pmp_val_stats).
        batch_range = (lo, hi): only batches lo .. hi-1 of the set's batches run (a rank's share, parallel.shard_bounds of the batch
        count; hi == lo runs nothing), and what comes back is not the list but the raw material of validation_numbers: (S
        float64[hi-lo,20], the batches' sizes).  The ranges' S and sizes, joined in batch order, give the whole run's numbers, bit for bit.
        return_confusion: one confusion call per batch beside the statistics call; the LAST element returned is then the confusion
        counts int64[7,5,5] of the whole set (pmp_val_confusion; see confusion_summary) - with batch_range the per-batch counts
        int64[hi-lo,7,5,5], whose sum over all ranges is the whole set's."""
        return _val_tuple(validation.run(self, "qbd", comp, qp, blocks, qt8, msbt, msdire, batch_size, logits, return_block_stats, batch_range,
                                         return_confusion), return_block_stats, batch_range is not None, return_confusion)

    def pre_validation(self, comp, qp, pred_id, blocks, qt8, msbt=None, msdire=None, batch_size=200, logits=None, return_block_stats=False,
                       batch_range=None, return_confusion=False):
        """Metrics.pre_validation (Metrics.py:196-274).  pred_id 0: the QT net alone -> [L1, accuracy], on pmp_infer_q_device: only the
        QT net is loaded and run, as in the reference, which never touches an MTT net here.  pred_id 1: the MTT net,
        TEACHER-FORCED with the QT label map float(qt8 - 1) (u8 subtraction: raw 0 -> 255.0) -> the reference's list of 13: [b0_L1, b1_L1,
        b2_L1, d0_L1, d1_L1, d2_L1, b0_accu, b1_accu, b2_accu, d0_accu, d1_accu, d2_accu, val_loss].  Batching, logits,
        return_block_stats, batch_range and return_confusion as in validation_QBD (logits = (qt,) for pred_id 0, (bt, dire) for pred_id 1;
        the confusion counts of the maps the mode does not predict are zero).  pred_id 2 belongs to a
        direction net the reference's Model_QBD.py no longer has: ValueError."""
        if pred_id not in (0, 1):
            raise ValueError("pre_validation: pred_id must be 0 (QT net) or 1 (MTT net, teacher-forced)")
        return _val_tuple(validation.run(self, validation.mode_of_pred(pred_id), comp, qp, blocks, qt8, msbt, msdire, batch_size, logits,
                                         return_block_stats, batch_range, return_confusion), return_block_stats, batch_range is not None, return_confusion)

    # ------------------------------------------------------------------------------------------ device API
    def infer_device(self, comp, qp, d_by, d_bu, d_bv, n, d_qt, d_bt, d_dire):
        self._ck(self.lib.pmp_infer_device(self.h, COMP_ID[comp], int(qp), d_by, d_bu, d_bv, int(n), d_qt, d_bt, d_dire))

    def infer_q_device(self, comp, qp, d_by, d_bu, d_bv, n, d_qt):
        """pmp_infer_q_device: the QT net alone; needs only the QT net of (comp, qp) loaded (load_q)."""
        self._ck(self.lib.pmp_infer_q_device(self.h, COMP_ID[comp], int(qp), d_by, d_bu, d_bv, int(n), d_qt))

    def postprocess_device(self, comp, d_qt, d_bt, d_dire, n, d_hor, d_ver, d_q8, d_d8):
        self._ck(self.lib.pmp_postprocess_device(self.h, COMP_ID[comp], d_qt, d_bt, d_dire, int(n), d_hor, d_ver, d_q8, d_d8))

    def infer_postprocess_device(self, comp, qp, d_by, d_bu, d_bv, n, d_hor, d_ver, d_q8, d_d8, d_qt=None, d_bt=None, d_dire=None):
        self._ck(self.lib.pmp_infer_postprocess_device(self.h, COMP_ID[comp], int(qp), d_by, d_bu, d_bv, int(n), d_hor, d_ver, d_q8,
                                                       d_d8, d_qt, d_bt, d_dire))

    def infer_postprocess_records_device(self, comp, qp, d_by, d_bu, d_bv, n, d_rec):
        """Blocks in, one packed 1344-byte record per block out (hor | ver | qt | dire): what the multi-GPU gather moves."""
        self._ck(self.lib.pmp_infer_postprocess_records_device(self.h, COMP_ID[comp], int(qp), d_by, d_bu, d_bv, int(n), d_rec))

    def postprocess_records_device(self, comp, d_qt, d_bt, d_dire, n, d_rec):
        self._ck(self.lib.pmp_postprocess_records_device(self.h, COMP_ID[comp], d_qt, d_bt, d_dire, int(n), d_rec))

    def cut_blocks_device(self, d_y, d_u, d_v, F, H, Wd, bitdepth, d_by, d_bu, d_bv):
        self._ck(self.lib.pmp_cut_blocks_device(self.h, d_y, d_u, d_v, int(F), int(H), int(Wd), int(bitdepth), d_by, d_bu, d_bv))

    # ------------------------------------------------------------------------------------------ timing
    def ktime_enable(self, mask):
        self._ck(self.lib.pmp_ktime_enable(self.h, int(mask)))

    def ktime(self):
        """{class name: (launches, total ms, algorithmic FLOPs)} accumulated since ktime_enable()."""
        out = {}
        for k in range(self.lib.pmp_ktime_classes()):
            n, ms, fl = C.c_int64(), C.c_double(), C.c_double()
            self._ck(self.lib.pmp_ktime_get(self.h, k, C.byref(n), C.byref(ms), C.byref(fl)))
            out[self.lib.pmp_ktime_name(k).decode()] = (n.value, ms.value, fl.value)
        return out

    # ------------------------------------------------------------------------------------------ helpers
    @staticmethod
    def _check_blocks(comp, by, bu, bv):
        if comp not in COMP_ID:
            raise ValueError("comp must be 'Luma' or 'Chroma'")
        if by.ndim != 3 or by.shape[1:] != (68, 68):
            raise ValueError("block_y must be u8[N,68,68]")
        n = by.shape[0]
        if comp == "Chroma":
            if bu is None or bv is None or bu.shape != (n, 34, 34) or bv.shape != (n, 34, 34):
                raise ValueError("Chroma needs block_u and block_v u8[N,34,34]")
        return n


def _val_tuple(run, want_blocks, ranged, want_confusion):
    """A validation.ValRun as validation_QBD / pre_validation document their returns - the one place where those tuple forms exist;
    ranged: batch_range was given."""
    if ranged:
        return (run.S, run.ns, run.conf) if want_confusion else (run.S, run.ns)
    out = (run.numbers(),) + ((run.block_stats,) if want_blocks else ()) + ((run.confusion(),) if want_confusion else ())
    return out[0] if len(out) == 1 else out


LOSS_KEYS = ("lambq", "lambb0", "lambb1", "lambb2", "lambd0", "lambd1", "lambd2", "lambresb0", "lambresb1", "lambresb2")


def loss_params(params=None):
    """-> _lib.LossParams from None (Train_QBD's defaults, Train_QBD.py:448-457), a dict with any of LOSS_KEYS, a text such as
    "lambb0=0.8,lambresb2=0" (pmp_parse_loss_params) or a LossParams.  An unknown key or a value that is not finite: ValueError."""
    if isinstance(params, _lib.LossParams):
        return params
    p = _lib.LossParams(1.0, (0.8, 1.0, 1.2), (1.0, 1.0, 1.0), (0.5, 0.5, 0.5))
    if params is None:
        return p
    if isinstance(params, dict):
        bad = [k for k in params if k not in LOSS_KEYS]
        if bad:
            raise ValueError("loss_params: unknown key %s (one of %s)" % (bad[0], ", ".join(LOSS_KEYS)))
        params = ",".join("%s=%r" % (k, float(v)) for k, v in params.items())
    if _lib.load().pmp_parse_loss_params(str(params).encode(), C.byref(p)) != 0:
        raise ValueError(_lib.load().pmp_last_error(None).decode())
    return p


def grad_bucket_floats(counts):
    """pmp_grad_bucket_floats (host only, no GPU): the gradient bucket of tensors of counts[i] floats -> (the bucket's floats, a multiple
    of 4; the tensors' offsets in floats, each a multiple of 4).  ValueError for an empty table or a count outside 1 .. 2^30 - 1."""
    nt = len(counts)
    if any(not -(1 << 63) <= int(k) < (1 << 63) for k in counts):
        raise ValueError("grad_bucket_floats: a count outside int64")
    off = (C.c_int64 * max(nt, 1))()
    total = _lib.load().pmp_grad_bucket_floats(nt, (C.c_int64 * max(nt, 1))(*[int(k) for k in counts]), off)
    if total < 0:
        raise ValueError("grad_bucket_floats: at least one tensor, every count in 1 .. 2^30 - 1")
    return int(total), [int(v) for v in off[:nt]]


def output_block_partition_map(file_path, frm_width, frm_height, frm_num, block_size=64, isChroma=False, return_unknown=False):
    """CreateDataSet.output_block_partition_map (CreateDataSet.py:188-264) through the host-only C parser (pmp_read_depth_dump; no GPU):
    the Save_Depth_fal dump of the patched VTM decoder -> qtdepth_block u8[n,8,8] (raw qtDepth), btdepth_block u8[n,16,16],
    msdirection_block i8[n,3,16,16], n = frm_num * (frm_height // 64) * (frm_width // 64).  return_unknown: also the number of unknown
    split codes (the reference prints "Error!!" for each).  PmpError(PMP_E_INVALID) where the reference would index wrongly or crash."""
    if int(block_size) != 64:
        raise ValueError("output_block_partition_map: block_size must be 64 (the nets' block)")
    lib = _lib.load()
    F, H, Wd = int(frm_num), int(frm_height), int(frm_width)
    n = max(F, 0) * (max(H, 0) // 64) * (max(Wd, 0) // 64)
    q = np.empty((n, 8, 8), np.uint8); b = np.empty((n, 16, 16), np.uint8); d = np.empty((n, 3, 16, 16), np.int8)
    unk = C.c_int64(0)
    _lib.check(lib.pmp_read_depth_dump(str(file_path).encode(), F, H, Wd, int(bool(isChroma)), _ptr(q), _ptr(b), _ptr(d), C.byref(unk)))
    return (q, b, d, unk.value) if return_unknown else (q, b, d)


def params_dict(p):
    d = {k: float(p.lamb[i]) for i, k in enumerate(PARAM_KEYS[:5])}
    d["thd"] = float(p.thd)
    return d


def parse_partition_params(spec, base=None):
    """'lamb1=0.6,thd=0.45' on top of `base` (a dict as get_partition_params returns; default: the reference's defaults) through the
    library's host-only parser (pmp_parse_partition_params: same keys, same domain check); needs no GPU.  PmpError on bad text."""
    lib = _lib.load()
    b = dict(DEFAULT_PARTITION_PARAMS, **(base or {}))
    p = _lib.PartitionParams()
    for i, k in enumerate(PARAM_KEYS[:5]):
        p.lamb[i] = b[k]
    p.thd = b["thd"]
    _lib.check(lib.pmp_parse_partition_params(str(spec).encode(), C.byref(p)))
    return params_dict(p)


def write_partition_file(path, frames, height, width, hor, ver, qt_u8, dire_i8):
    """Map2Partition.py:385-412 (tiling + text emission) through the C writer; host-only, needs no GPU."""
    lib = _lib.load()
    hor = np.ascontiguousarray(hor, np.uint8); ver = np.ascontiguousarray(ver, np.uint8)
    q8 = np.ascontiguousarray(qt_u8, np.uint8); d8 = np.ascontiguousarray(dire_i8, np.int8)
    n = int(frames) * (int(height) // 64) * (int(width) // 64)
    if hor.size != n * 256 or ver.size != n * 256 or q8.size != n * 64 or d8.size != n * 768:
        raise ValueError("write_partition_file: array sizes do not match frames*(H//64)*(W//64) blocks")
    _lib.check(lib.pmp_write_partition_file(str(path).encode(), int(frames), int(height), int(width), _ptr(hor), _ptr(ver), _ptr(q8), _ptr(d8)))


def write_partition_binary(path, frames, height, width, hor, ver, qt_u8, dire_i8):
    """Binary side channel of the same data (include/pmp.h): frame matrices as the VTM keeps them."""
    lib = _lib.load()
    hor = np.ascontiguousarray(hor, np.uint8); ver = np.ascontiguousarray(ver, np.uint8)
    q8 = np.ascontiguousarray(qt_u8, np.uint8); d8 = np.ascontiguousarray(dire_i8, np.int8)
    n = int(frames) * (int(height) // 64) * (int(width) // 64)
    if hor.size != n * 256 or ver.size != n * 256 or q8.size != n * 64 or d8.size != n * 768:
        raise ValueError("write_partition_binary: array sizes do not match frames*(H//64)*(W//64) blocks")
    _lib.check(lib.pmp_write_partition_binary(str(path).encode(), int(frames), int(height), int(width), _ptr(hor), _ptr(ver), _ptr(q8), _ptr(d8)))


def tile_partition_maps(frames, height, width, hor, ver, qt_u8, dire_i8):
    """Per-block flags -> the frame matrices the patched VTM keeps after parsing (EncAppCfg.cpp:4270-4298): hor, ver
    u8[F][R][C], qt u8[F][R/2][C/2], dire i8[F][3][R][C], R = 16*(H>>6), C = 16*(W>>6) (pmp_tile_partition_maps)."""
    lib = _lib.load()
    R, Cc = 16 * (height // 64), 16 * (width // 64)
    hor, ver, qt_u8 = _u8(hor), _u8(ver), _u8(qt_u8)
    dire_i8 = np.ascontiguousarray(dire_i8, dtype=np.int8)
    oh = np.zeros((frames, R, Cc), np.uint8); ov = np.zeros_like(oh)
    oq = np.zeros((frames, R // 2, Cc // 2), np.uint8); od = np.zeros((frames, 3, R, Cc), np.int8)
    rc = lib.pmp_tile_partition_maps(frames, height, width, _ptr(hor), _ptr(ver), _ptr(qt_u8), _ptr(dire_i8), _ptr(oh), _ptr(ov),
                                     _ptr(oq), _ptr(od))
    if rc != 0:
        raise _lib.PmpError(rc, lib.pmp_last_error(None).decode())
    return oh, ov, oq, od


def read_partition_binary(path):
    """-> (frames, height, width, hor[F,R,C] u8, ver[F,R,C] u8, qt[F,R/2,C/2] u8, dire[F,3,R,C] i8) via numpy.memmap."""
    raw = np.memmap(path, dtype=np.uint8, mode="r")
    if bytes(raw[:8]) != b"PMPB1\0\0\0":
        raise ValueError("%s: not a PMPB1 file" % path)
    frames, H, Wd, R, Cc = (int(v) for v in np.frombuffer(raw[8:28].tobytes(), dtype="<i4"))
    per = 5 * R * Cc + R * Cc // 4
    body = raw[40:40 + frames * per].reshape(frames, per)
    hor = body[:, :R * Cc].reshape(frames, R, Cc); ver = body[:, R * Cc:2 * R * Cc].reshape(frames, R, Cc)
    qt = body[:, 2 * R * Cc:2 * R * Cc + R * Cc // 4].reshape(frames, R // 2, Cc // 2)
    dire = body[:, 2 * R * Cc + R * Cc // 4:].reshape(frames, 3, R, Cc).view(np.int8)
    return frames, H, Wd, hor, ver, qt, dire


def format_partition_text(frames, height, width, hor, ver, qt_u8, dire_i8):
    lib = _lib.load()
    hor = np.ascontiguousarray(hor, np.uint8); ver = np.ascontiguousarray(ver, np.uint8)
    q8 = np.ascontiguousarray(qt_u8, np.uint8); d8 = np.ascontiguousarray(dire_i8, np.int8)
    need = _lib.check(lib.pmp_format_partition_text(int(frames), int(height), int(width), _ptr(hor), _ptr(ver), _ptr(q8), _ptr(d8), None, 0))
    buf = C.create_string_buffer(max(int(need), 1))
    got = _lib.check(lib.pmp_format_partition_text(int(frames), int(height), int(width), _ptr(hor), _ptr(ver), _ptr(q8), _ptr(d8), buf, need))
    assert got == need
    return buf.raw[:need]


def format_partition_rows_records(width, block_rows, rec):
    """Text of `block_rows` consecutive block rows of one frame from packed records u8[block_rows * (width // 64), 1344]
    (pmp_format_partition_rows_records): -> (ctypes char buffer holding the six sections back to back, int64[block_rows, 6] exact
    byte count of every (block row, section)).  Host-only; the C formatter releases the GIL."""
    lib = _lib.load()
    rec = np.ascontiguousarray(rec, np.uint8)
    bw = int(width) // 64
    if rec.size != int(block_rows) * bw * _lib.PMP_RECORD_BYTES:
        raise ValueError("format_partition_rows_records: %d bytes of records for %d block rows of %d blocks" % (rec.size, block_rows, bw))
    sizes = np.zeros((int(block_rows), 6), np.int64)
    need = _lib.check(lib.pmp_format_partition_rows_records(int(width), int(block_rows), _ptr(rec), None, 0, _ptr(sizes)))
    buf = C.create_string_buffer(max(int(need), 1))
    got = _lib.check(lib.pmp_format_partition_rows_records(int(width), int(block_rows), _ptr(rec), buf, need, None))
    assert got == need == int(sizes.sum())
    return buf, sizes


def tile_partition_rows_records(width, block_rows, rec):
    """The same rows as matrices: hor, ver u8[16 n, C], qt u8[8 n, C/2], dire i8[3, 16 n, C] (pmp_tile_partition_rows_records)."""
    lib = _lib.load()
    rec = np.ascontiguousarray(rec, np.uint8)
    R, Cc = 16 * int(block_rows), 16 * (int(width) // 64)
    if rec.size != int(block_rows) * (Cc // 16) * _lib.PMP_RECORD_BYTES:
        raise ValueError("tile_partition_rows_records: record count does not match the geometry")
    oh = np.zeros((R, Cc), np.uint8); ov = np.zeros_like(oh); oq = np.zeros((R // 2, Cc // 2), np.uint8); od = np.zeros((3, R, Cc), np.int8)
    if rec.size:
        _lib.check(lib.pmp_tile_partition_rows_records(int(width), int(block_rows), _ptr(rec), _ptr(oh), _ptr(ov), _ptr(oq), _ptr(od)))
    return oh, ov, oq, od


def read_partition_file(path, frames, height, width):
    """Parser with the geometry rules of EncAppCfg::parsePartitionMatrix (EncAppCfg.cpp:4247-4250, :4299-4399):
    returns hor, ver [F,R,C], qt [F,R/2,C/2], dire [F,3,R,C] as int arrays (frame matrices, not per block)."""
    vals = np.array(open(path).read().split(), dtype=np.int64)
    R, Cc = (height >> 6) * 16, (width >> 6) * 16
    per = 5 * R * Cc + R * Cc // 4
    if vals.size != frames * per:
        raise ValueError("%s: %d values, expected %d" % (path, vals.size, frames * per))
    v = vals.reshape(frames, per)
    hor = v[:, :R * Cc].reshape(frames, R, Cc); ver = v[:, R * Cc:2 * R * Cc].reshape(frames, R, Cc)
    qt = v[:, 2 * R * Cc:2 * R * Cc + R * Cc // 4].reshape(frames, R // 2, Cc // 2)
    dire = v[:, 2 * R * Cc + R * Cc // 4:].reshape(frames, 3, R, Cc)
    return hor, ver, qt, dire
