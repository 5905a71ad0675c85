"""libvpx.opencl_amd -- MI355X-native VP8 decode pixel path (host-side Python plumbing).

The product is the two native libraries built from ``csrc/``:

* ``lib/libvp8hip.so``  -- hand-written HIP kernels for gfx950 + the C-ABI shim (``include/vp8hip.h``)
* ``lib/libvpx_hip.so`` -- the C host side: bitstream feeder (``vp8_parser``), decoder core and the
  ``vpx_codec`` / ``vp8_dx`` interface (``include/vpx/*.h``), linked against ``libvp8hip.so``

This module only binds them with ctypes for the tests and ``bench.py`` (the reference is C; the
drop-in boundary is the C ABI, Python is plumbing).  It deliberately has NO CPU fallback:
``Vp8Hip()`` raises if the HIP library or a gfx950 device is missing.

The directory name contains a dot, so it is loaded by path (see ``__graft_entry__.load_package``).
"""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIBDIR = os.path.join(HERE, "lib")
HIP_LIB = os.environ.get("VP8HIP_LIB") or os.path.join(LIBDIR, "libvp8hip.so")      # (VP8HIP_LIB: a diagnostic variant, tools/variant.sh)
HOST_LIB = os.path.join(LIBDIR, "libvpx_hip.so")

c_void_p, c_int, c_size_t = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t

STAGE_RECON, STAGE_LF, STAGE_EXTEND, STAGE_ALL = 1, 2, 4, 7


def build(verbose=False):
    """Compile every native piece in-tree (hipcc cross-compiles gfx950 without a GPU)."""
    out = subprocess.run(["make", "-C", os.path.join(HERE, "csrc"), "all"], capture_output=True, text=True)
    if out.returncode:
        raise RuntimeError("native build failed:\n" + out.stdout + out.stderr)
    if verbose:
        print(out.stdout)


# ------------------------------------------------------------------------------------------
# IR structures (include/vp8_ir.h)
# ------------------------------------------------------------------------------------------
class FrameHdr(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint16), ("height", ctypes.c_uint16), ("mb_cols", ctypes.c_uint16),
                ("mb_rows", ctypes.c_uint16), ("frame_type", ctypes.c_uint8), ("version", ctypes.c_uint8),
                ("show_frame", ctypes.c_uint8), ("filter_type", ctypes.c_uint8), ("filter_level", ctypes.c_uint8),
                ("sharpness_level", ctypes.c_uint8), ("segmentation_enabled", ctypes.c_uint8),
                ("mb_segment_abs_delta", ctypes.c_uint8), ("segment_quant", ctypes.c_int8 * 4),
                ("segment_lf", ctypes.c_int8 * 4), ("mode_ref_lf_delta_enabled", ctypes.c_uint8),
                ("ref_lf_deltas", ctypes.c_int8 * 4), ("mode_lf_deltas", ctypes.c_int8 * 4),
                ("base_qindex", ctypes.c_uint8), ("y1dc_delta_q", ctypes.c_int8), ("y2dc_delta_q", ctypes.c_int8),
                ("y2ac_delta_q", ctypes.c_int8), ("uvdc_delta_q", ctypes.c_int8), ("uvac_delta_q", ctypes.c_int8),
                ("refresh_last", ctypes.c_uint8), ("refresh_golden", ctypes.c_uint8), ("refresh_alt", ctypes.c_uint8),
                ("copy_buffer_to_gf", ctypes.c_uint8), ("copy_buffer_to_arf", ctypes.c_uint8),
                ("sign_bias_golden", ctypes.c_uint8), ("sign_bias_alt", ctypes.c_uint8),
                ("color_space", ctypes.c_uint8), ("clamping_type", ctypes.c_uint8),
                ("num_token_partitions", ctypes.c_uint8), ("lf_key_frame", ctypes.c_uint8), ("rsv", ctypes.c_uint8 * 14)]


assert ctypes.sizeof(FrameHdr) == 64


class EntropyFrame(ctypes.Structure):
    """vp8hip_entropy_frame (include/vp8hip.h): what the host's header parse hands to the device's entropy decoder."""
    _fields_ = [("hdr", FrameHdr), ("data_off", ctypes.c_uint64), ("first_pos", ctypes.c_uint32), ("first_end", ctypes.c_uint32),
                ("first_value", ctypes.c_uint32), ("first_bits", ctypes.c_int32), ("first_range", ctypes.c_uint32),
                ("num_tok", ctypes.c_uint32), ("tok_pos", ctypes.c_uint32 * 8), ("tok_end", ctypes.c_uint32 * 8),
                ("update_mb_segmentation_map", ctypes.c_uint8), ("mb_no_coeff_skip", ctypes.c_uint8),
                ("prob_skip_false", ctypes.c_uint8), ("segmap_keep", ctypes.c_uint8), ("segment_tree_probs", ctypes.c_uint8 * 3),
                ("rsv1", ctypes.c_uint8), ("coef_probs", ctypes.c_uint8 * 1056),
                ("prob_intra", ctypes.c_uint8), ("prob_last", ctypes.c_uint8), ("prob_gf", ctypes.c_uint8), ("rsv2", ctypes.c_uint8),
                ("ymode_prob", ctypes.c_uint8 * 4), ("uvmode_prob", ctypes.c_uint8 * 3), ("rsv3", ctypes.c_uint8),
                ("mvc", ctypes.c_uint8 * 38), ("rsv4", ctypes.c_uint8 * 2), ("rsv5", ctypes.c_uint8 * 4)]


class Geom(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("aligned_w", "aligned_h", "y_stride", "uv_stride", "y_plane_size",
                                     "uv_plane_size", "frame_size", "y_off", "u_off", "v_off")]


def geom(width, height):
    """vp8ir_geom_init (include/vp8_ir.h) restated for numpy-side indexing."""
    g = Geom()
    aw, ah = (width + 15) & ~15, (height + 15) & ~15
    g.aligned_w, g.aligned_h = aw, ah
    g.y_stride = (aw + 64 + 31) & ~31
    g.uv_stride = g.y_stride >> 1
    g.y_plane_size = (ah + 64) * g.y_stride
    g.uv_plane_size = (ah // 2 + 32) * g.uv_stride
    g.frame_size = g.y_plane_size + 2 * g.uv_plane_size
    g.y_off = 32 * g.y_stride + 32
    g.u_off = g.y_plane_size + 16 * g.uv_stride + 16
    g.v_off = g.y_plane_size + g.uv_plane_size + 16 * g.uv_stride + 16
    return g


class Refs(ctypes.Structure):
    _fields_ = [("new_idx", c_int), ("lst_idx", c_int), ("gld_idx", c_int), ("alt_idx", c_int),
                ("ref_cnt", c_int * 4), ("show_idx", c_int)]


class Job(ctypes.Structure):
    _fields_ = [("ir_slot", ctypes.c_int32), ("dst_fb", ctypes.c_int32), ("ref_fb", ctypes.c_int32 * 4)]


class Stats(ctypes.Structure):
    _fields_ = [("recon_ms", ctypes.c_float), ("lf_ms", ctypes.c_float), ("extend_ms", ctypes.c_float),
                ("recon_waves", c_int), ("lf_waves", c_int), ("workgroups", c_int), ("detile_pass", c_int),
                ("lf_kernels", c_int), ("fused", c_int), ("pred_tiles", c_int)]


# ------------------------------------------------------------------------------------------
# IVF container + MD5 of a decoded frame (vpxdec.c:386-441 / examples/decode_to_md5.txt:28-47)
# ------------------------------------------------------------------------------------------
def read_ivf(path):
    data = open(path, "rb").read()
    if len(data) < 32 or data[:4] != b"DKIF":
        raise ValueError(f"{path}: not an IVF file")
    w, h = int.from_bytes(data[12:14], "little"), int.from_bytes(data[14:16], "little")
    frames, pos = [], 32
    while pos + 12 <= len(data):
        sz = int.from_bytes(data[pos:pos + 4], "little")
        pos += 12
        if pos + sz > len(data):
            break
        frames.append(data[pos:pos + sz])
        pos += sz
    return w, h, frames


def frame_md5(buf, g, width, height):
    """MD5 over the visible Y, U, V rows of a whole frame buffer (numpy uint8, vp8ir_geom layout)."""
    m = hashlib.md5()
    cw, ch = (width + 1) // 2, (height + 1) // 2
    for off, stride, w, h in ((g.y_off, g.y_stride, width, height), (g.u_off, g.uv_stride, cw, ch),
                              (g.v_off, g.uv_stride, cw, ch)):
        plane = np.lib.stride_tricks.as_strided(buf[off:], shape=(h, w), strides=(stride, 1))
        m.update(np.ascontiguousarray(plane).tobytes())
    return m.hexdigest()


def planes_md5(y, u, v):
    m = hashlib.md5()
    for p in (y, u, v):
        m.update(np.ascontiguousarray(p).tobytes())
    return m.hexdigest()


# ------------------------------------------------------------------------------------------
# host feeder (vp8_parser.h), exported by libvpx_hip.so
# ------------------------------------------------------------------------------------------
_host = None


def load_host():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise RuntimeError(f"{HOST_LIB} missing: run __graft_entry__.build()")
        # libvpx_hip.so links libvp8hip.so (rpath $ORIGIN)
        L = ctypes.CDLL(HOST_LIB)
        L.vp8_parser_create.restype = c_void_p
        L.vp8_parser_destroy.argtypes = [c_void_p]
        L.vp8_parser_set_threads.argtypes = [c_void_p, c_int]
        L.vp8_parser_set_device_segmap.argtypes = [c_void_p, c_int]
        L.vp8_parser_set_error_concealment.argtypes = [c_void_p, c_int]
        L.vp8_parser_conceals.argtypes = [c_void_p]
        L.vp8_parser_frame_hdr.argtypes = [c_void_p, c_void_p]
        L.vp8_parser_begin_frame.argtypes = [c_void_p, ctypes.c_char_p, c_size_t, c_void_p]
        L.vp8_parser_decode_mbs.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        L.vp8_parser_decode_mbs_compact.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, ctypes.POINTER(c_size_t), c_void_p, c_void_p]
        L.vp8_parser_export_entropy.argtypes = [c_void_p, c_void_p]
        L.vp8_parser_error.argtypes = [c_void_p]
        L.vp8_parser_error.restype = ctypes.c_char_p
        for f in ("vp8_refs_init", "vp8_refs_on_alloc", "vp8_refs_release_new"):
            getattr(L, f).argtypes = [c_void_p]
        L.vp8_refs_get_free.argtypes = [c_void_p]
        L.vp8_refs_swap.argtypes = [c_void_p, c_void_p]
        _host = L
    return _host


class Parser:
    """Bitstream -> IR.  Owns the reference-buffer bookkeeping too (vp8_refs)."""

    def __init__(self):
        self.L = load_host()
        self.p = c_void_p(self.L.vp8_parser_create())
        self.refs = Refs()
        self.L.vp8_refs_init(ctypes.byref(self.refs))
        self.dims = None
        self._undo = None

    def close(self):
        if self.p:
            self.L.vp8_parser_destroy(self.p)
            self.p = None

    def set_threads(self, n):
        """token partitions of a frame on up to n threads (vp8_parser_set_threads)"""
        self.L.vp8_parser_set_threads(self.p, n)

    def set_device_segmap(self, on=True):
        """the device keeps this stream's segment map, in the IR slot its frames are decoded into (vp8_parser_set_device_segmap)"""
        self.L.vp8_parser_set_device_segmap(self.p, int(on))

    def final_hdr(self, hdr):
        """after decode_mbs: the header as the pixel path is to see it (vp8_parser_frame_hdr)"""
        self.L.vp8_parser_frame_hdr(self.p, ctypes.byref(hdr))
        return hdr

    def set_error_concealment(self, on=True):
        """before the first frame: conceal lost frames and lost residuals (vp8_parser_set_error_concealment)"""
        self.L.vp8_parser_set_error_concealment(self.p, int(on))

    def begin(self, data):
        """-> (hdr, dims_changed).  Acquires refs.new_idx like the reference's get_free_fb."""
        hdr = FrameHdr()
        self._undo = None
        before = Refs.from_buffer_copy(self.refs), self.dims
        if self.L.vp8_refs_get_free(ctypes.byref(self.refs)) < 0:
            raise RuntimeError("no free frame buffer")
        self._frame_data = data          # the parser borrows the compressed frame until decode_mbs has run (vp8_parser.h)
        rc = self.L.vp8_parser_begin_frame(self.p, data, len(data), ctypes.byref(hdr))
        if rc:
            self.L.vp8_refs_release_new(ctypes.byref(self.refs))
            raise ValueError(f"vp8 header error {rc}: {self.L.vp8_parser_error(self.p).decode()}")
        changed = self.dims != (hdr.width, hdr.height)
        if changed:
            self.dims = (hdr.width, hdr.height)
            self.L.vp8_refs_on_alloc(ctypes.byref(self.refs))
        self._undo = before
        return hdr, changed

    def abandon(self):
        """The frame begin() opened is not going to be decoded now: the bookkeeping goes back to what it was before begin() -- the
        buffer it took is free again and, where the frame brought a new size, neither the size nor the reallocation has
        happened -- so that begin() on the same frame does all of it again (and reports the change of size again)."""
        if self._undo is not None:
            saved, self.dims = self._undo
            ctypes.memmove(ctypes.byref(self.refs), ctypes.byref(saved), ctypes.sizeof(Refs))
            self._undo = None

    def export_entropy(self):
        """After begin() on a key frame: the frame's vp8hip_entropy_frame (offsets relative to the frame's first byte); the
        parser is done with the frame.  None when the frame is not one the device decodes (it stays open for decode_mbs)."""
        out = EntropyFrame()
        rc = self.L.vp8_parser_export_entropy(self.p, ctypes.byref(out))
        if rc == 5:
            return None
        if rc:
            self.L.vp8_refs_release_new(ctypes.byref(self.refs))
            raise ValueError(f"vp8 header error {rc}: {self.L.vp8_parser_error(self.p).decode()}")
        return out

    def decode_mbs(self, mbs_ptr, coef_ptr, mvs_ptr):
        corrupt = c_int(0)
        rc = self.L.vp8_parser_decode_mbs(self.p, mbs_ptr, coef_ptr, mvs_ptr, ctypes.byref(corrupt))
        if rc:
            self.L.vp8_refs_release_new(ctypes.byref(self.refs))
            raise ValueError(f"vp8 macroblock data error {rc}: {self.L.vp8_parser_error(self.p).decode()}")
        return corrupt.value

    def decode_mbs_compact(self, mbx_ptr, blocks_ptr, cap_blocks, mvs_ptr):
        """The macroblocks in the DEVICE FORM of include/vp8_ir.h (records + block stream) -> (blocks written, corrupt flag)"""
        corrupt, nb = c_int(0), c_size_t(0)
        rc = self.L.vp8_parser_decode_mbs_compact(self.p, mbx_ptr, blocks_ptr, cap_blocks, ctypes.byref(nb), mvs_ptr, ctypes.byref(corrupt))
        if rc:
            self.L.vp8_refs_release_new(ctypes.byref(self.refs))
            raise ValueError(f"vp8 macroblock data error {rc}: {self.L.vp8_parser_error(self.p).decode()}")
        return nb.value, corrupt.value

    def swap(self, hdr):
        self.L.vp8_refs_swap(ctypes.byref(self.refs), ctypes.byref(hdr))


def parse_to_numpy_compact(parser, data):
    """One frame in the device form -> (hdr, mbx uint8[n,128], blocks int16[nb,16], mvs int16[n,16,2], corrupt)."""
    hdr, changed = parser.begin(data)
    n = hdr.mb_cols * hdr.mb_rows
    mbx = np.zeros((n, 128), np.uint8)
    blocks = np.zeros((n * 24, 16), np.int16)
    mvs = np.zeros((n, 16, 2), np.int16)
    nb, corrupt = parser.decode_mbs_compact(mbx.ctypes.data, blocks.ctypes.data, n * 24, mvs.ctypes.data)
    return hdr, mbx, blocks[:nb].copy(), mvs, corrupt


def block_kinds(mbs):
    """vp8ir_block_kind for every block of every macroblock: uint8[n, 25] of 0 (nothing), 1 (a lone first coefficient), 2 (more).
    mbs: uint8[n, >=64] descriptors."""
    ymode, flags, eobs = mbs[:, 0], mbs[:, 3], mbs[:, 8:33]
    has_y2 = (ymode != 4) & (ymode != 9)
    kind = np.zeros(eobs.shape, np.uint8)
    kind[eobs == 1] = 1
    kind[eobs > 1] = 2
    kind[:, :16][(eobs[:, :16] == 1) & has_y2[:, None]] = 0
    kind[~has_y2, 24] = 0
    kind[(flags & 1) != 0] = 0
    return kind


def compact_from_dense(mbs, coef):
    """The device form of include/vp8_ir.h (vp8ir_compact_mb restated with numpy): (mbx uint8[n,128], blocks int16[nb,16])."""
    n = mbs.shape[0]
    kind = block_kinds(mbs)
    c = coef.reshape(n, 25, 16)
    mbx = np.zeros((n, 128), np.uint8)
    mbx[:, :64] = mbs[:, :64]
    full = kind[:, :24] == 2
    first = np.concatenate(([0], np.cumsum(full.sum(1))[:-1])).astype(np.uint32)
    mbx[:, 56:60] = first.view(np.uint8).reshape(n, 4)
    mbx[:, 60:64] = 0
    aux = np.zeros((n, 32), np.int16)
    has_y2 = (mbs[:, 0] != 4) & (mbs[:, 0] != 9)
    skip = (mbs[:, 3] & 1) != 0
    y2rows = has_y2 & ~skip & (mbs[:, 8 + 24] != 0)
    aux[y2rows, :16] = c[y2rows, 24, :]
    lone = kind[:, :24] == 1
    dc = c[:, :24, 0]
    aux[:, :16] = np.where(lone[:, :16], dc[:, :16], aux[:, :16])
    aux[:, 16:24] = np.where(lone[:, 16:24], dc[:, 16:24], 0)
    mbx[:, 64:128] = aux.view(np.uint8).reshape(n, 64)
    return mbx, np.ascontiguousarray(c[:, :24][full])


def dense_from_compact(mbx, blocks):
    """vp8ir_expand_mb restated with numpy: (mbs uint8[n,64] with sparse_first cleared, coef int16[n,400])."""
    n = mbx.shape[0]
    mbs = mbx[:, :64].copy()
    first = mbs[:, 56:60].copy().view(np.uint32).reshape(n)
    mbs[:, 56:64] = 0
    kind = block_kinds(mbs)
    aux = mbx[:, 64:128].copy().view(np.int16).reshape(n, 32)
    c = np.zeros((n, 25, 16), np.int16)
    has_y2 = (mbs[:, 0] != 4) & (mbs[:, 0] != 9)
    skip = (mbs[:, 3] & 1) != 0
    y2rows = has_y2 & ~skip & (mbs[:, 8 + 24] != 0)
    c[y2rows, 24, :] = aux[y2rows, :16]
    lone = kind[:, :24] == 1
    c[:, :16, 0] = np.where(lone[:, :16], aux[:, :16], 0)
    c[:, 16:24, 0] = np.where(lone[:, 16:24], aux[:, 16:24], 0)
    full = kind[:, :24] == 2
    rank = np.cumsum(full, 1) - full
    idx = first[:, None] + rank
    c[:, :24][full] = blocks[idx[full]]
    return mbs, c.reshape(n, 400)


def parse_to_numpy(parser, data):
    """One frame -> (hdr, mbs uint8[n,64], coef int16[n,400], mvs int16[n,16,2]) in numpy arrays."""
    hdr, changed = parser.begin(data)
    n = hdr.mb_cols * hdr.mb_rows
    mbs = np.zeros((n, 64), np.uint8)
    coef = np.zeros((n, 400), np.int16)
    mvs = np.zeros((n, 16, 2), np.int16)
    parser.decode_mbs(mbs.ctypes.data, coef.ctypes.data, mvs.ctypes.data)
    return hdr, changed, mbs, coef, mvs


def i420_size(w, h):
    """bytes of a packed I420 frame: w * h + 2 * ((w + 1) / 2) * ((h + 1) / 2)"""
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


def split_i420(t, w, h):
    """Y [.., h, w], U and V [.., (h + 1) / 2, (w + 1) / 2] views of packed I420 frames t [..., i420_size(w, h)] (numpy or torch)"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    lead = tuple(t.shape[:-1])
    y = t[..., :w * h].reshape(lead + (h, w))
    u = t[..., w * h:w * h + cw * ch].reshape(lead + (ch, cw))
    v = t[..., w * h + cw * ch:w * h + 2 * cw * ch].reshape(lead + (ch, cw))
    return y, u, v


RGB_MATRICES = {"bt601": 0, "bt601-full": 1, "bt709": 2}       # VP8HIP_RGB_BT601 ...
RGB_LAYOUTS = {"nchw": 0, "nhwc": 1, "nhwc4": 2}                # VP8HIP_RGB_PLANAR, PACKED3, PACKED4
RGB_ORDERS = {"rgb": 0, "bgr": 1}
RGB_U8, RGB_F16, RGB_F32 = 0, 1, 2


def rgb_size(w, h, layout="nchw", dtype=RGB_U8):
    """bytes of one frame of Vp8Hip.frames_rgb (vp8hip_rgb_size): w * h * channels * element size; 0 for a size outside 1..16383,
    an unknown layout / type, or "nhwc4" with a float type.  dtype: RGB_U8 / RGB_F16 / RGB_F32 or the torch / numpy type's name"""
    dt = _elem_dtype(dtype, _RGB_DTYPES)
    if layout not in RGB_LAYOUTS or dt is None or not (1 <= w <= 16383 and 1 <= h <= 16383) or (layout == "nhwc4" and dt != RGB_U8):
        return 0
    return w * h * (4 if layout == "nhwc4" else 3) * (1, 2, 4)[dt]


_RGB_DTYPES = ("uint8", "float16", "float32")                 # by RGB_U8, RGB_F16, RGB_F32
_INT16_DTYPES = ("int16", "float16", "float32")                # by SIDE_I16 ... and RES_I16 ...


def _elem_dtype(dtype, names):
    """a tensor type's number -- itself, or the torch / numpy type's name looked up in `names` -- or None for one that is not there"""
    if isinstance(dtype, int):
        return dtype if 0 <= dtype < len(names) else None
    name = str(dtype).split(".")[-1]
    return names.index(name) if name in names else None


SIDE_PLANES = {"ref": 1, "mode": 2, "skip": 4, "segment": 8, "qindex": 16, "coded": 32}      # VP8HIP_SIDE_*: bit order = plane order
SIDE_I16, SIDE_F16, SIDE_F32 = 0, 1, 2


def _plane_mask(planes, table, allow_empty):
    """names of `table` (any order; the tensor's planes come in bit order) or the mask itself -> the mask, None for an unknown plane
    and, unless allow_empty, for none"""
    if isinstance(planes, int):
        return planes if (0 if allow_empty else 1) <= planes <= sum(table.values()) else None
    mask = 0
    for name in planes:
        if name not in table:
            return None
        mask |= table[name]
    return mask if mask or allow_empty else None


def side_sizes(gw, gh, mv_dtype=SIDE_I16, planes=("ref", "mode", "skip")):
    """(bytes of one frame's mv tensor, bytes of its info tensor) of Vp8Hip.frames_side on a grid of gw x gh (vp8hip_side_mv_size,
    vp8hip_side_info_size): 2 * gh * gw * element size and planes * gh * gw; (0, 0) for a size outside 1..16383, an unknown type or
    plane.  For the native grid gw, gh = 4 * mb_cols, 4 * mb_rows."""
    dt, mask = _elem_dtype(mv_dtype, _INT16_DTYPES), _plane_mask(planes, SIDE_PLANES, True)
    if dt is None or mask is None or gw == 0 or gh == 0:         # (0 x 0 would ask for the native grid, which needs a context)
        return 0, 0
    L, p = load_hip(), SideParams(int(gw), int(gh), dt, mask)
    return int(L.vp8hip_side_mv_size(None, ctypes.byref(p))), int(L.vp8hip_side_info_size(None, ctypes.byref(p)))


def trace_size(w, h):
    """bytes of one trace of Vp8Hip.frames_trace at a display size of w x h (vp8hip_trace_size): a dword per pixel"""
    return 4 * int(w) * int(h)


def trace_residual_size(gw, gh, dtype=0):
    """bytes of one frame's tensor of Vp8Hip.trace_residual on a grid of gw x gh (vp8hip_trace_residual_size): 3 * gh * gw elements;
    0 for a size outside 1..16383 or an unknown type.  dtype: RES_I16 / RES_F16 / RES_F32 or the torch / numpy type's name.  For the
    display size pass the display size."""
    dt = _elem_dtype(dtype, _INT16_DTYPES)
    if dt is None or gw == 0 or gh == 0:         # (0 x 0 would ask for the display size, which needs a context)
        return 0
    p = TraceResidualParams(int(gw), int(gh), 0, 0, dt)
    return int(load_hip().vp8hip_trace_residual_size(None, ctypes.byref(p)))


WEAR_PLANES = {"hops": 1, "intra": 2, "edge": 4, "coded": 8}   # VP8HIP_WEAR_*: bit order = plane order = the counter's byte
WEAR_U8, WEAR_F16, WEAR_F32 = 0, 1, 2


def _entry_tensor_size(gw, gh, planes, dtype, table, params, size):
    """what trace_wear_size and trace_cover_size are: planes of `table`, the ctypes struct and the library's size call"""
    dt, mask = _elem_dtype(dtype, _RGB_DTYPES), _plane_mask(planes, table, False)
    if dt is None or mask is None or gw == 0 or gh == 0:         # (0 x 0 would ask for the display size, which needs a context)
        return 0
    p = params(int(gw), int(gh), dt, mask)
    return int(getattr(load_hip(), size)(None, ctypes.byref(p)))


def trace_wear_size(gw, gh, planes=("hops", "intra", "edge", "coded"), dtype=0):
    """bytes of one frame's tensor of Vp8Hip.trace_wear on a grid of gw x gh (vp8hip_trace_wear_size): planes * gh * gw elements; 0 for
    a size outside 1..16383, an unknown type, no plane or an unknown one.  dtype: WEAR_U8 / WEAR_F16 / WEAR_F32 or the torch / numpy
    type's name.  For the display size pass the display size."""
    return _entry_tensor_size(gw, gh, planes, dtype, WEAR_PLANES, TraceWearParams, "vp8hip_trace_wear_size")


COVER_PLANES = {"count": 1, "seen": 2}                        # VP8HIP_COVER_*: bit order = plane order


def trace_cover_size(gw, gh, planes=("count", "seen"), dtype=0):
    """bytes of one frame's tensor of Vp8Hip.trace_cover on a grid of gw x gh (vp8hip_trace_cover_size): planes * gh * gw elements; 0
    for a size outside 1..16383, an unknown type, no plane or an unknown one.  dtype: WEAR_U8 / WEAR_F16 / WEAR_F32 or the torch /
    numpy type's name.  For the display size pass the display size."""
    return _entry_tensor_size(gw, gh, planes, dtype, COVER_PLANES, TraceCoverParams, "vp8hip_trace_cover_size")


HIST_PLANES = {"y": 1, "u": 2, "v": 4}                       # VP8HIP_HIST_Y, _U, _V: bit order = plane order
SLOT_HIST_PLANES = dict(SIDE_PLANES, mvmag=64)                # VP8HIP_SIDE_* and VP8HIP_HIST_MVMAG, for Vp8Hip.slots_hist only


def hist_size(planes):
    """bytes of one output of Vp8Hip.frames_hist, slots_hist, trace_wear_hist and trace_cover_hist (vp8hip_hist_size): 1024 a plane,
    256 uint32 counts; 0 for no plane.  planes: how many there are, or their names"""
    if isinstance(planes, (tuple, list, set, frozenset)):
        planes = len(set(planes))
    elif not isinstance(planes, int):
        return 0
    return int(load_hip().vp8hip_hist_size(int(planes)))


SSIM_F16, SSIM_F32 = 1, 2                                    # VP8HIP_SSIM_F16, _F32
_SSIM_DTYPES = (None, "float16", "float32")                   # by VP8HIP_SSIM_*: 0 is no map


def _ssim_dtype(map_dtype):
    """a map type's number -- SSIM_F16 / SSIM_F32 or the torch / numpy type's name -- or None for anything else"""
    dt = _elem_dtype(map_dtype, _SSIM_DTYPES)
    return dt if dt in (SSIM_F16, SSIM_F32) else None


def ssim_windows(w, h):
    """(nwx, nwy): the windows Vp8Hip.frames_ssim has in a plane of w x h (vp8hip_ssim_windows; on the host, no GPU): vp8_ssim2's 8x8
    windows on the 4-pixel grid, the last aligned one left out as the reference leaves it out -- (w - 5) // 4 columns for w > 8, else
    none, and likewise rows.  ValueError for a size outside 1..16383."""
    nwx, nwy = c_int(), c_int()
    if load_hip().vp8hip_ssim_windows(int(w), int(h), ctypes.byref(nwx), ctypes.byref(nwy)):
        raise ValueError(f"ssim_windows: {w}x{h}: refused (sizes 1..16383)")
    return nwx.value, nwy.value


def _ssim_plane_windows(w, h, planes):
    """-> [(nwx, nwy)] of the planes of `planes` ("y", "u", "v" or the mask) of a picture of w x h, in bit order; a plane that lacks
    windows one way has none: (0, 0); None for no plane or an unknown one"""
    mask = _plane_mask(planes, HIST_PLANES, False)
    if mask is None:
        return None
    out = []
    for b in range(3):
        if mask >> b & 1:
            nwx, nwy = ssim_windows((w + 1) // 2 if b else w, (h + 1) // 2 if b else h)
            out.append((nwx, nwy) if nwx and nwy else (0, 0))
    return out


def ssim_sizes(w, h, planes=("y", "u", "v"), map_dtype=None):
    """(bytes of one job's scores, bytes of its map) of Vp8Hip.frames_ssim at a display size of w x h (vp8hip_ssim_scores_size, and
    what vp8hip_ssim_map_size gives on a context of that size): 16 a plane, and the planes' windows back to back in map_dtype
    (SSIM_F16 / SSIM_F32 or the torch / numpy type's name; None: no map, 0 bytes).  (0, 0) for no plane or an unknown one, or an
    unknown type."""
    wins = _ssim_plane_windows(int(w), int(h), planes)
    dt = None if map_dtype is None else _ssim_dtype(map_dtype)
    if wins is None or (map_dtype is not None and dt is None):
        return 0, 0
    return int(load_hip().vp8hip_ssim_scores_size(len(wins))), 0 if dt is None else sum(a * b for a, b in wins) * (0, 2, 4)[dt]


def split_ssim_map(t, w, h, planes=("y", "u", "v")):
    """the flat map [n, elems] of Vp8Hip.frames_ssim at a display size of w x h -> a list of views [n, nwy, nwx], one per plane asked
    for, in bit order (a plane without windows: [n, 0, 0])"""
    wins = _ssim_plane_windows(int(w), int(h), planes)
    if wins is None or t.ndim != 2 or t.shape[1] != sum(a * b for a, b in wins):
        raise ValueError(f"split_ssim_map: planes {planes!r} of {w}x{h} are not a map of {tuple(t.shape)}")
    out, off = [], 0
    for nwx, nwy in wins:
        out.append(t[:, off:off + nwx * nwy].reshape(t.shape[0], nwy, nwx))
        off += nwx * nwy
    return out


MOTION_PLANES = {"sad": 1, "sad0": 2, "sse": 4, "var": 8, "srcvar": 16}      # VP8HIP_MOTION_*: bit order = plane order
MOTION_MAX_DISTANCE = 64


def motion_sizes(mb_cols, mb_rows, planes=("sad",)):
    """(bytes of one job's mv tensor, bytes of its stats) of Vp8Hip.frames_motion on a grid of mb_cols x mb_rows macroblocks (what
    vp8hip_motion_mv_size and vp8hip_motion_stats_size give on a context of that size): int16 [2, mb_rows, mb_cols] -- the centre
    tensor's size too -- and uint32 [P, mb_rows, mb_cols]; the latter 0 for no plane or an unknown one, both 0 for an empty grid"""
    mask = _plane_mask(planes, MOTION_PLANES, True)
    cells = int(mb_cols) * int(mb_rows)
    if int(mb_cols) < 1 or int(mb_rows) < 1:
        return 0, 0
    return 4 * cells, 0 if not mask else 4 * bin(mask).count("1") * cells


SUBPEL_PLANES = {"val": 1, "var": 2, "sse": 4, "var0": 8}      # VP8HIP_SUBPEL_*: bit order = plane order
SUBPEL_MAX_COST_RANGE = 1023
SUBPEL_MAX_ERROR_PER_BIT = 16383


def subpel_sizes(mb_cols, mb_rows, planes=("val",)):
    """(bytes of one job's mv tensor, bytes of its stats) of Vp8Hip.frames_subpel on a grid of mb_cols x mb_rows macroblocks (what
    vp8hip_subpel_mv_size and vp8hip_subpel_stats_size give on a context of that size): int16 [2, mb_rows, mb_cols] -- the start and
    the ref tensor's size too -- and uint32 [P, mb_rows, mb_cols]; the latter 0 for no plane or an unknown one, both 0 for an empty
    grid"""
    mask = _plane_mask(planes, SUBPEL_PLANES, True)
    cells = int(mb_cols) * int(mb_rows)
    if int(mb_cols) < 1 or int(mb_rows) < 1:
        return 0, 0
    return 4 * cells, 0 if not mask else 4 * bin(mask).count("1") * cells


TFILTER_FILTERS = {"sixtap": 0, "bilinear": 1}                # VP8HIP_TFILTER_SIXTAP, _BILINEAR
TFILTER_MAX_COUNT = 15                                        # sources a job: the reference's arnr_max_frames


def tfilter_sizes(w, h):
    """(bytes of one job's picture, bytes of its count plane) of Vp8Hip.frames_tfilter at the display size w x h: packed I420 in
    uint8 (vp8hip_i420_size) and the same geometry in uint16 (vp8hip_tfilter_count_size); both 0 for a size outside 1..16383"""
    if not (1 <= int(w) <= 16383 and 1 <= int(h) <= 16383):
        return 0, 0
    size = i420_size(int(w), int(h))
    return size, 2 * size


QUANT_QUANTIZERS = {"regular": 0, "fast": 1}                  # VP8HIP_QUANT_REGULAR, _FAST
QUANT_PLANES = {"erry": 1, "erry2": 2, "erruv": 4, "eobs": 8, "recsse": 16}      # VP8HIP_QUANT_*: bit order = plane order
QUANT_ZBIN_MAX = 1 << 20                                      # the largest |zbin_over_quant|, |zbin_mode_boost|, |act_zbin_adj|


def quant_sizes(w, h, planes=()):
    """(bytes of one job's coef records, of its eobs, of its stats, of its reconstruction) of Vp8Hip.frames_quant at the display
    size w x h: int16 [mb_rows, mb_cols, 25, 16], uint8 [mb_rows, mb_cols, 32], uint32 [P, mb_rows, mb_cols] (0 for no plane or an
    unknown one) and packed I420 (vp8hip_i420_size); all 0 for a size outside 1..16383"""
    if not (1 <= int(w) <= 16383 and 1 <= int(h) <= 16383):
        return 0, 0, 0, 0
    cells = ((int(w) + 15) // 16) * ((int(h) + 15) // 16)
    mask = _plane_mask(planes, QUANT_PLANES, True)
    return 800 * cells, 32 * cells, 0 if not mask else 4 * bin(mask).count("1") * cells, i420_size(int(w), int(h))


def quant_factors(qindex, deltas=(0, 0, 0, 0, 0)):
    """what the reference's vp8cx_init_quantizer computes with improved_quant for one qindex (vp8hip_quant_factors; on the host, no
    GPU): a dict of int16 arrays [3, 2] -- Y1, Y2, UV by dc, ac -- "quant", "quant_shift", "quant_fast", "zbin", "round", "dequant",
    and "zrun_zbin_boost" [3, 16].  deltas: y1dc, y2dc, y2ac, uvdc, uvac, each -15..15"""
    d = [int(v) for v in deltas]
    if len(d) != 5:
        raise ValueError("quant_factors: five deltas (y1dc, y2dc, y2ac, uvdc, uvac)")
    t = QuantTable()
    if load_hip().vp8hip_quant_factors(int(qindex), (c_int * 5)(*d), ctypes.byref(t)):
        raise ValueError(f"quant_factors: qindex {qindex} (0..127), deltas {deltas!r} (-15..15)")
    return {name: np.ctypeslib.as_array(getattr(t, name)).copy() for name, _ in QuantTable._fields_}


PACK_OVERFLOW, PACK_BAD_VECTOR, PACK_BAD_LEVEL, PACK_CLAMPS = 1, 2, 4, 8      # VP8HIP_PACK_*: the status bits of Vp8Hip.frames_pack
PACK_BAD_MODE = 16                                            # VP8HIP_PACK_BAD_MODE: frames_pack_key's, beside OVERFLOW and BAD_LEVEL
INTRA_PLANES = {"rd16": 1, "rd4": 2, "rate": 4, "eobs": 8, "recsse": 16}        # VP8HIP_INTRA_*: bit order = plane order
INTRA_NO_BPRED = 1                                            # VP8HIP_INTRA_NO_BPRED


def intra_sizes(w, h, planes=()):
    """(bytes of one job's coef records, of its eobs, of its stats, of its reconstruction, of its modes) of Vp8Hip.frames_intra at the
    display size w x h: 800, 32, 4 * planes and 32 bytes a macroblock, and i420_size(w, h); (0, 0, 0, 0, 0) for a size outside
    1..16383 or an unknown plane"""
    mask = _plane_mask(planes, INTRA_PLANES, True)
    if mask is None or not (1 <= w <= 16383 and 1 <= h <= 16383):
        return 0, 0, 0, 0, 0
    n = ((w + 15) // 16) * ((h + 15) // 16)
    return 800 * n, 32 * n, 4 * bin(mask).count("1") * n, int(load_hip().vp8hip_i420_size(int(w), int(h))), 32 * n


def intra_costs():
    """the reference's key-frame mode costs (vp8hip_intra_costs; on the host, no GPU): (mbmode_cost int32 [5] -- DC, V, H, TM, B_PRED --,
    bmode_cost int32 [10, 10, 10] -- above, left, mode), as vp8_init_mode_costs computes them"""
    t = IntraCost()
    if load_hip().vp8hip_intra_costs(ctypes.byref(t)):
        raise ValueError("intra_costs: refused")
    return np.ctypeslib.as_array(t.mbmode_cost).astype(np.int32), np.ctypeslib.as_array(t.bmode_cost).astype(np.int32).reshape(10, 10, 10)


def intra_rd(qindex, y1dc_delta=0, zbin_over_quant=0):
    """(rdmult, rddiv) of the reference's vp8_initialize_rd_consts for one pass (vp8hip_intra_rd; on the host, no GPU)"""
    m, d = c_int(), c_int()
    if load_hip().vp8hip_intra_rd(int(qindex), int(y1dc_delta), int(zbin_over_quant), ctypes.byref(m), ctypes.byref(d)):
        raise ValueError(f"intra_rd: qindex {qindex} (0..127), y1dc_delta {y1dc_delta} (-15..15)")
    return m.value, d.value


# what Vp8Hip.frames_pack and pack_header take beside the levels, the vectors and the quantiser, with their defaults
PACK_DEFAULTS = dict(version=0, show_frame=1, filter_type=0, filter_level=0, sharpness=0, ref_frame=1, refresh_last=1, refresh_golden=0, refresh_alt=0,
                     copy_buffer_to_gf=0, copy_buffer_to_arf=0, sign_bias_golden=0, sign_bias_alt=0, log2_parts=0, prob_skip_false=200, prob_intra=150,
                     prob_last=140, prob_gf=100)


def _pack_params(who, qindex, deltas, fields, n=None, key=False):
    """-> (PackParams -- key: PackKeyParams --, the array job_qindex points to -- to be kept alive -- or None); ValueError for an
    unknown field or a wrong count"""
    defaults = PACK_KEY_DEFAULTS if key else PACK_DEFAULTS
    unknown = set(fields) - set(defaults)
    if unknown:
        raise ValueError(f"{who}: unknown parameters {sorted(unknown)!r} (of {', '.join(defaults)})")
    d = [int(v) for v in deltas]
    if len(d) != 5:
        raise ValueError(f"{who}: five deltas (y1dc, y2dc, y2ac, uvdc, uvac)")
    p = PackKeyParams() if key else PackParams()
    for name, v in {**defaults, **fields}.items():
        setattr(p, name, int(v))
    p.delta = (c_int * 5)(*d)
    jq = None
    if isinstance(qindex, (int, np.integer)):
        p.qindex = int(qindex)
    else:
        qs = [int(q) for q in qindex]
        if n is None or len(qs) != n:
            raise ValueError(f"{who}: {len(qs)} qindex values for {n} jobs")
        if any(not 0 <= q <= 127 for q in qs):
            raise ValueError(f"{who}: qindex {qindex!r} (0..127)")
        jq = (ctypes.c_uint8 * n)(*qs)
        p.qindex, p.job_qindex = qs[0], jq
    return p, jq


def _pack_bound(w, h, log2_parts, header, first):
    """the bound of a frame with `header` bytes before the first partition and at most `first` bytes a macroblock in it"""
    if not (1 <= int(w) <= 16383 and 1 <= int(h) <= 16383 and 0 <= int(log2_parts) <= 3):
        return 0
    cells, parts = ((int(w) + 15) // 16) * ((int(h) + 15) // 16), 1 << int(log2_parts)
    return (header + (64 + 8 + first * cells) + 3 * (parts - 1) + 6672 * cells + 4 * parts + 15) // 16 * 16


def _pack_head_dict(h):
    """a PackHead as the dict the three header functions return"""
    out = {name: int(getattr(h, name)) for name in ("bottom", "range", "bit_count", "cache", "pending", "settled")}
    out["bytes"] = bytes(h.bytes[:h.nbytes])
    return out


def pack_bound(w, h, log2_parts=0):
    """a `cap` that always suffices for a frame of Vp8Hip.frames_pack at the display size w x h: what vp8hip_pack_bound gives for a
    context of that size (include/vp8hip.h derives it: 7 bits a put, 32 puts a macroblock in the first partition, 7625 in the
    tokens); 0 for a size outside 1..16383 or log2_parts outside 0..3"""
    return _pack_bound(w, h, log2_parts, 3, 28)


def pack_header(qindex=40, deltas=(0, 0, 0, 0, 0), **fields):
    """the frame header of Vp8Hip.frames_pack's frames through the library's C bool encoder, up to where the per-macroblock data
    begin (vp8hip_pack_header; on the host, no GPU): a dict of "bytes" -- what the coder has written by then --, "bottom", "range",
    "bit_count" -- its state -- and "cache", "pending", "settled", the same in the form the device continues from.  fields:
    PACK_DEFAULTS' names"""
    p, _ = _pack_params("pack_header", 0, deltas, fields)
    h = PackHead()
    if load_hip().vp8hip_pack_header(ctypes.byref(p), int(qindex), ctypes.byref(h)):
        raise ValueError(f"pack_header: qindex {qindex} (0..127), deltas {deltas!r} (-15..15) or {fields!r} out of range")
    return _pack_head_dict(h)


ADAPT_COEF, ADAPT_MV, ADAPT_SKIP, ADAPT_REF = 1, 2, 4, 8     # VP8HIP_ADAPT_*: what Vp8Hip.frames_pack_adapt fits to the frame's counts
ADAPT_ALL = 15
PACK_PROBS_BYTES = 1104                                       # sizeof(vp8hip_pack_probs): coef [4][8][3][11], mvc [2][19], 10 reserved
PACK_COUNTS = 1216                                            # a job's counts: token counts [4][8][3][12], then 2 x 32 vector branch counts


def pack_probs_default():
    """the default probability set of Vp8Hip.frames_pack_adapt (vp8hip_pack_probs_default; on the host): uint8 [1104] --
    vp8_default_coef_probs [4][8][3][11], vp8_default_mv_context [2][19], 10 reserved bytes of 0"""
    out = np.zeros(PACK_PROBS_BYTES, np.uint8)
    load_hip().vp8hip_pack_probs_default(c_void_p(out.ctypes.data))
    return out


def pack_adapt_bound(w, h, log2_parts=0):
    """a `cap` that always suffices for a frame of Vp8Hip.frames_pack_adapt at the display size w x h (vp8hip_pack_adapt_bound):
    pack_bound plus 8624 bytes, the worst case of the header's probability section; 0 where pack_bound is 0"""
    b = pack_bound(w, h, log2_parts)
    return b + 8624 if b else 0


def pack_header_prefix(qindex=40, deltas=(0, 0, 0, 0, 0), refresh_entropy_probs=1, **fields):
    """the frame header of Vp8Hip.frames_pack_adapt's frames through refresh_last, where the probability section begins
    (vp8hip_pack_header_prefix; on the host, no GPU): a dict as pack_header's"""
    p, _ = _pack_params("pack_header_prefix", 0, deltas, fields)
    h = PackHead()
    if load_hip().vp8hip_pack_header_prefix(ctypes.byref(p), int(qindex), int(refresh_entropy_probs), ctypes.byref(h)):
        raise ValueError(f"pack_header_prefix: qindex {qindex} (0..127), deltas {deltas!r} (-15..15), refresh_entropy_probs "
                         f"{refresh_entropy_probs} (0, 1) or {fields!r} out of range")
    return _pack_head_dict(h)


def pack_frames(data, info):
    """(data, info) of Vp8Hip.frames_pack or frames_pack_key (torch tensors or arrays) -> a list of each job's compressed frame as
    bytes, None where the job's status has PACK_OVERFLOW, PACK_BAD_VECTOR, PACK_BAD_LEVEL or PACK_BAD_MODE"""
    d = np.asarray(data.cpu() if hasattr(data, "cpu") else data)
    i = np.asarray(info.cpu() if hasattr(info, "cpu") else info)
    fatal = PACK_OVERFLOW | PACK_BAD_VECTOR | PACK_BAD_LEVEL | PACK_BAD_MODE
    return [None if int(s[0]) & fatal else d[k, :int(s[1])].tobytes() for k, s in enumerate(i)]


# what Vp8Hip.frames_pack_key and pack_key_header take beside the modes, the levels and the quantiser, with their defaults
PACK_KEY_DEFAULTS = dict(version=0, show_frame=1, color_space=0, clamping_type=0, filter_type=0, filter_level=0, sharpness=0, log2_parts=0,
                         prob_skip_false=200)


def pack_key_bound(w, h, log2_parts=0):
    """a `cap` that always suffices for a frame of Vp8Hip.frames_pack_key at the display size w x h: what vp8hip_pack_key_bound gives
    for a context of that size (include/vp8hip.h derives it: 7 bits a put, 117 puts a macroblock in the first partition, 7625 in
    the tokens, ten bytes of frame header); 0 for a size outside 1..16383 or log2_parts outside 0..3"""
    return _pack_bound(w, h, log2_parts, 10, 103)


def pack_key_header(qindex=40, deltas=(0, 0, 0, 0, 0), **fields):
    """the frame header of Vp8Hip.frames_pack_key's frames through the library's C bool encoder, up to where the per-macroblock
    data begin (vp8hip_pack_key_header; on the host, no GPU): a dict as pack_header's.  fields: PACK_KEY_DEFAULTS' names"""
    p, _ = _pack_params("pack_key_header", 0, deltas, fields, key=True)
    h = PackHead()
    if load_hip().vp8hip_pack_key_header(ctypes.byref(p), int(qindex), ctypes.byref(h)):
        raise ValueError(f"pack_key_header: qindex {qindex} (0..127), deltas {deltas!r} (-15..15) or {fields!r} out of range")
    return _pack_head_dict(h)


def ssim_mean(scores):
    """the scores [n, P, 2] of Vp8Hip.frames_ssim (a torch tensor or an array) -> float64 [n, P]: total / 2^32 / count, what
    vp8_ssim2 returns to within 2^-33 + N * 2^-52; NaN where the count is 0 (the reference's 0 / 0)"""
    s = np.asarray(scores.cpu() if hasattr(scores, "cpu") else scores).astype(np.int64)
    if s.ndim < 1 or s.shape[-1] != 2:
        raise ValueError("ssim_mean: scores are [..., 2]: total, count")
    total, count = s[..., 0].astype(np.float64), s[..., 1].astype(np.float64)     # (|total| < 2^57: the conversion rounds, 2^-53 relative)
    out = np.full(total.shape, np.nan)
    np.divide(total / 4294967296.0, count, out=out, where=count != 0)
    return out


def ssim_combined(means, how="ssimg"):
    """the per-plane means [..., 3] (Y, U, V) as one figure, by the two weightings of vp8/encoder/ssim.c: "ssimg" = (4a + b + c) / 6
    (vp8_calc_ssimg), "ssim" = 0.8a + 0.1(b + c) (vp8_calc_ssim)"""
    m = np.asarray(means, np.float64)
    if m.ndim < 1 or m.shape[-1] != 3 or how not in ("ssimg", "ssim"):
        raise ValueError("ssim_combined: means [..., 3] and \"ssimg\" or \"ssim\"")
    a, b, c = m[..., 0], m[..., 1], m[..., 2]
    return (a * 4 + b + c) / 6 if how == "ssimg" else a * 0.8 + 0.1 * (b + c)


GATHER_FILTERS = {"nearest": 0, "bilinear": 1}              # VP8HIP_GATHER_NEAREST, BILINEAR
GATHER_LAYOUTS = {"planar": 0, "channels_last": 1}            # VP8HIP_GATHER_PLANAR, CHANNELS_LAST


def trace_gather_size(gw, gh, channels, elem, src_w=1, src_h=1, layout="planar", filter="nearest"):
    """bytes of one output of Vp8Hip.trace_gather on a grid of gw x gh (vp8hip_trace_gather_size): channels * gh * gw * elem; 0 for a
    size or a source grid outside 1..16383, channels outside 1..4096, an element size other than 1, 2 or 4, an unknown layout or filter,
    or "bilinear" on 1-byte elements.  For the display size pass the display size."""
    if layout not in GATHER_LAYOUTS or filter not in GATHER_FILTERS or gw == 0 or gh == 0:     # (0 x 0 would ask for the display size)
        return 0
    p = TraceGatherParams(int(gw), int(gh), int(src_w), int(src_h), int(channels), int(elem), GATHER_LAYOUTS[layout], GATHER_FILTERS[filter])
    return int(load_hip().vp8hip_trace_gather_size(None, ctypes.byref(p)))


RES_LAYOUTS = {"i420": 0, "planar": 1}                        # VP8HIP_RES_I420, PLANAR
RES_I16, RES_F16, RES_F32 = 0, 1, 2


def residual_sizes(gw, gh, dtype=RES_I16, layout="planar"):
    """bytes of one frame's tensor of Vp8Hip.frames_residual on a grid of gw x gh (vp8hip_residual_size): 3 * gh * gw elements
    ("planar") or gh * gw + 2 * ((gh + 1) / 2) * ((gw + 1) / 2) ("i420"); 0 for a size outside 1..16383, an unknown type or layout.
    For the native grid gw, gh = 16 * mb_cols, 16 * mb_rows."""
    dt = _elem_dtype(dtype, _INT16_DTYPES)
    if dt is None or layout not in RES_LAYOUTS or gw == 0 or gh == 0:       # (0 x 0 would ask for the native grid, which needs a context)
        return 0
    p = ResidualParams(int(gw), int(gh), RES_LAYOUTS[layout], dt)
    return int(load_hip().vp8hip_residual_size(None, ctypes.byref(p)))


def split_residual(t, gw, gh):
    """Y [.., gh, gw], U and V [.., (gh + 1) / 2, (gw + 1) / 2] views of "i420" residual frames t [..., elements] (numpy or torch),
    as split_i420 splits pictures"""
    return split_i420(t, gw, gh)


COEF_STAGES = {"dequant": 0, "levels": 1}                     # VP8HIP_COEF_DEQUANT, LEVELS
COEF_LAYOUTS = {"channels": 0, "inplace": 1}                  # VP8HIP_COEF_CHANNELS, INPLACE
COEF_ORDERS = {"raster": 0, "zigzag": 1}                      # VP8HIP_COEF_RASTER, ZIGZAG
COEF_PLANES = {"y": 1, "u": 2, "v": 4, "y2": 8}               # VP8HIP_COEF_*: bit order = plane order
COEF_CELLS = {"y": 4, "u": 2, "v": 2, "y2": 1}                # blocks of a macroblock each way
COEF_ZIGZAG = (0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15)     # channel j of "zigzag" is position COEF_ZIGZAG[j] = 4 * v + u


def _coef_params(stage, layout, planes, nfreq, order, dtype):
    """-> (CoefParams, its dtype number, its plane mask), or None for names the tables do not have.  (Numbers go through as they
    are: the library judges them.)"""
    dt, mask = _elem_dtype(dtype, _INT16_DTYPES), _plane_mask(planes, COEF_PLANES, False)
    if dt is None or mask is None or stage not in COEF_STAGES or layout not in COEF_LAYOUTS or order not in COEF_ORDERS:
        return None
    return CoefParams(COEF_STAGES[stage], COEF_LAYOUTS[layout], COEF_ORDERS[order], int(nfreq), mask, dt), dt, mask


def coef_size(ctx, stage="dequant", layout="channels", planes=("y", "u", "v"), nfreq=16, order="raster", dtype=RES_I16):
    """bytes of one frame's tensor of Vp8Hip.frames_coef on context `ctx`, a Vp8Hip (vp8hip_coef_size): the planes asked for, each
    nfreq * (G * mb_rows) * (G * mb_cols) elements with G = 4, 2, 2, 1 for "y", "u", "v", "y2" ("inplace": nfreq is 16); 0 for what
    the call refuses -- an unknown stage, layout, order, type or plane, no plane, nfreq outside 1..16, "inplace" with nfreq below 16
    or "zigzag" -- and for ctx None: there is only the native grid, which is the context's."""
    made = _coef_params(stage, layout, planes, nfreq, order, dtype)
    if made is None:
        return 0
    return int(load_hip().vp8hip_coef_size(None if ctx is None else ctx.h, ctypes.byref(made[0])))


def split_coef(t, mb_cols, mb_rows, layout="channels", planes=("y", "u", "v"), nfreq=16):
    """{plane: view} of coefficient frames t [..., elements] (numpy or torch) as Vp8Hip.frames_coef writes them, the planes back to
    back in bit order: "channels" [..., nfreq, G * mb_rows, G * mb_cols], "inplace" [..., 4 * G * mb_rows, 4 * G * mb_cols]"""
    mask = _plane_mask(planes, COEF_PLANES, False)
    if mask is None or layout not in COEF_LAYOUTS:
        raise ValueError(f"split_coef: planes {planes!r}, layout {layout!r}")
    views, at = {}, 0
    for name, bit in COEF_PLANES.items():
        if mask & bit:
            g = COEF_CELLS[name]
            shape = (int(nfreq), g * mb_rows, g * mb_cols) if layout == "channels" else (4 * g * mb_rows, 4 * g * mb_cols)
            size = int(np.prod(shape))
            views[name] = t[..., at:at + size].reshape(tuple(t.shape[:-1]) + shape)
            at += size
    if at != t.shape[-1]:
        raise ValueError(f"split_coef: {t.shape[-1]} elements a frame, the planes take {at}")
    return views


def dequant_factors(hdr):
    """int16 [4, 6]: y1dc, y1ac, y2dc, y2ac, uvdc, uvac of each segment for frame header `hdr` (vp8hip_dequant_factors; on the host, no
    GPU): what turns the "levels" of Vp8Hip.frames_coef into its "dequant" values -- but for the luma DCs of macroblocks with a Y2
    block, which come out of that block's inverse WHT."""
    out = np.zeros((4, 6), np.int16)
    if load_hip().vp8hip_dequant_factors(ctypes.byref(hdr), out.ctypes.data):
        raise ValueError("dequant_factors: refused")
    return out


# ------------------------------------------------------------------------------------------
# HIP pixel path (vp8hip.h)
# ------------------------------------------------------------------------------------------
_hip = None
_torch_first = None     # was torch imported before libvp8hip.so was loaded? (Vp8Hip.frames_scaled)


class PostprocParams(ctypes.Structure):     # vp8hip_pp, include/vp8hip.h
    _fields_ = [("flags", ctypes.c_int32), ("flimit", ctypes.c_int32), ("mb_flimit", ctypes.c_int32), ("rv_offset", ctypes.c_int32),
                ("noise_clamp", ctypes.c_int32), ("rv", c_void_p), ("noise", c_void_p), ("noise_rows", c_void_p)]


PP_DEBLOCK, PP_DEMACROBLOCK, PP_ADDNOISE = 1, 2, 4


class RgbParams(ctypes.Structure):          # vp8hip_rgb, include/vp8hip.h
    _fields_ = [("dst_w", c_int), ("dst_h", c_int), ("filter", c_int), ("matrix", c_int), ("layout", c_int), ("order", c_int),
                ("dtype", c_int), ("scale", ctypes.c_float * 3), ("bias", ctypes.c_float * 3)]


class SideParams(ctypes.Structure):         # vp8hip_side, include/vp8hip.h
    _fields_ = [("dst_w", c_int), ("dst_h", c_int), ("mv_dtype", c_int), ("planes", ctypes.c_uint), ("scale", ctypes.c_float * 2)]


class ResidualParams(ctypes.Structure):     # vp8hip_residual, include/vp8hip.h
    _fields_ = [("dst_w", c_int), ("dst_h", c_int), ("layout", c_int), ("dtype", c_int), ("scale", ctypes.c_float * 3)]


class CoefParams(ctypes.Structure):         # vp8hip_coef, include/vp8hip.h
    _fields_ = [("stage", c_int), ("layout", c_int), ("order", c_int), ("nfreq", c_int), ("planes", ctypes.c_uint), ("dtype", c_int),
                ("scale", ctypes.c_float * 4)]


class TraceFlowParams(ctypes.Structure):    # vp8hip_trace_flow, include/vp8hip.h
    _fields_ = [("dst_w", c_int), ("dst_h", c_int), ("dtype", c_int), ("scale", ctypes.c_float * 2)]


class AnchorJob(ctypes.Structure):          # vp8hip_anchor_job, include/vp8hip.h
    _fields_ = [("fb", ctypes.c_int32), ("trace", ctypes.c_int32), ("anchor_fb", ctypes.c_int32)]


class TraceResidualParams(ctypes.Structure):    # vp8hip_trace_residual, include/vp8hip.h
    _fields_ = [("dst_w", c_int), ("dst_h", c_int), ("matrix", c_int), ("order", c_int), ("dtype", c_int), ("scale", ctypes.c_float * 3)]


class GatherJob(ctypes.Structure):          # vp8hip_gather_job, include/vp8hip.h
    _fields_ = [("trace", ctypes.c_int32), ("src", ctypes.c_int32)]


class TraceGatherParams(ctypes.Structure):  # vp8hip_trace_gather, include/vp8hip.h
    _fields_ = [("dst_w", c_int), ("dst_h", c_int), ("src_w", c_int), ("src_h", c_int), ("channels", c_int), ("elem", c_int),
                ("layout", c_int), ("filter", c_int)]


class TraceWearParams(ctypes.Structure):    # vp8hip_trace_wear, include/vp8hip.h
    _fields_ = [("dst_w", c_int), ("dst_h", c_int), ("dtype", c_int), ("planes", ctypes.c_uint), ("scale", ctypes.c_float * 4)]


class InvertJob(ctypes.Structure):          # vp8hip_invert_job, include/vp8hip.h
    _fields_ = [("trace", ctypes.c_int32), ("dst", ctypes.c_int32)]


class TraceCoverParams(ctypes.Structure):   # vp8hip_trace_cover, include/vp8hip.h
    _fields_ = [("dst_w", c_int), ("dst_h", c_int), ("dtype", c_int), ("planes", ctypes.c_uint), ("scale", ctypes.c_float * 2)]


class HistJob(ctypes.Structure):            # vp8hip_hist_job, include/vp8hip.h
    _fields_ = [("fb", ctypes.c_int32), ("ref_fb", ctypes.c_int32)]


class SsimParams(ctypes.Structure):         # vp8hip_ssim, include/vp8hip.h
    _fields_ = [("planes", ctypes.c_uint), ("map_dtype", c_int)]


class MotionParams(ctypes.Structure):       # vp8hip_motion, include/vp8hip.h
    _fields_ = [("distance", c_int), ("sad_per_bit", c_int), ("planes", ctypes.c_uint), ("cost", ctypes.POINTER(ctypes.c_int32))]


class SubpelParams(ctypes.Structure):       # vp8hip_subpel, include/vp8hip.h
    _fields_ = [("precision", c_int), ("error_per_bit", c_int), ("cost_range", c_int), ("planes", ctypes.c_uint),
                ("cost", ctypes.POINTER(ctypes.c_int32))]


class TfilterParams(ctypes.Structure):      # vp8hip_tfilter, include/vp8hip.h
    _fields_ = [("strength", c_int), ("filter", c_int), ("thresh_low", ctypes.c_uint), ("thresh_high", ctypes.c_uint)]


class TfilterJob(ctypes.Structure):         # vp8hip_tfilter_job, include/vp8hip.h
    _fields_ = [("fb", ctypes.c_int32), ("first", ctypes.c_int32), ("count", ctypes.c_int32)]


class QuantTable(ctypes.Structure):         # vp8hip_quant_table, include/vp8hip.h
    _fields_ = [(name, ctypes.c_int16 * 2 * 3) for name in ("quant", "quant_shift", "quant_fast", "zbin", "round", "dequant")] + \
               [("zrun_zbin_boost", ctypes.c_int16 * 16 * 3)]


class QuantParams(ctypes.Structure):        # vp8hip_quant, include/vp8hip.h
    _fields_ = [("qindex", c_int), ("delta", c_int * 5), ("quantizer", c_int), ("filter", c_int), ("stage", c_int), ("zbin_over_quant", c_int),
                ("zbin_mode_boost", c_int), ("act_zbin_adj", c_int), ("planes", ctypes.c_uint), ("job_qindex", ctypes.POINTER(ctypes.c_uint8))]


class IntraCost(ctypes.Structure):          # vp8hip_intra_cost, include/vp8hip.h
    _fields_ = [("mbmode_cost", c_int * 5), ("bmode_cost", c_int * 10 * 10 * 10)]


class IntraParams(ctypes.Structure):        # vp8hip_intra, include/vp8hip.h
    _fields_ = [("q", QuantParams), ("rdmult", c_int), ("rddiv", c_int), ("bmode_last", c_int), ("flags", ctypes.c_uint), ("planes", ctypes.c_uint),
                ("cost", IntraCost)]


class PackParams(ctypes.Structure):         # vp8hip_pack, include/vp8hip.h
    _fields_ = [(name, c_int) for name in ("version", "show_frame", "filter_type", "filter_level", "sharpness", "qindex")] + [("delta", c_int * 5)] + \
               [(name, c_int) for name in ("ref_frame", "refresh_last", "refresh_golden", "refresh_alt", "copy_buffer_to_gf", "copy_buffer_to_arf",
                                           "sign_bias_golden", "sign_bias_alt", "log2_parts", "prob_skip_false", "prob_intra", "prob_last", "prob_gf")] + \
               [("job_qindex", ctypes.POINTER(ctypes.c_uint8))]


class PackKeyParams(ctypes.Structure):      # vp8hip_pack_key, include/vp8hip.h
    _fields_ = [(name, c_int) for name in ("version", "show_frame", "color_space", "clamping_type", "filter_type", "filter_level", "sharpness",
                                           "qindex")] + [("delta", c_int * 5), ("log2_parts", c_int), ("prob_skip_false", c_int),
                                                         ("job_qindex", ctypes.POINTER(ctypes.c_uint8))]


class PackHead(ctypes.Structure):           # vp8hip_pack_head, include/vp8hip.h
    _fields_ = [("bottom", ctypes.c_uint32), ("range", ctypes.c_uint32), ("bit_count", ctypes.c_uint32), ("nbytes", ctypes.c_uint32),
                ("cache", ctypes.c_int32), ("pending", ctypes.c_uint32), ("settled", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("bytes", ctypes.c_uint8 * 64)]


class PackAdapt(ctypes.Structure):          # vp8hip_pack_adapt, include/vp8hip.h
    _fields_ = [("flags", c_int), ("refresh_entropy_probs", c_int), ("probs_in", c_void_p), ("probs_in_stride", c_size_t)]


class VisParams(ctypes.Structure):         # vp8hip_vis, include/vp8hip.h
    _fields_ = [("flags", ctypes.c_uint), ("ref_frame_mask", c_int), ("mb_modes_mask", c_int), ("b_modes_mask", c_int),
                ("mv_mask", c_int), ("frame_info", ctypes.c_char_p), ("rate_info", ctypes.c_char_p)]


def load_hip():
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB):
            raise RuntimeError(f"{HIP_LIB} missing: run __graft_entry__.build(); there is no CPU fallback")
        L = ctypes.CDLL(HIP_LIB, mode=ctypes.RTLD_GLOBAL)
        L.vp8hip_create.argtypes = [c_int, ctypes.POINTER(c_void_p)]
        L.vp8hip_destroy.argtypes = [c_void_p]
        L.vp8hip_last_error.argtypes = [c_void_p]
        L.vp8hip_last_error.restype = ctypes.c_char_p
        L.vp8hip_configure.argtypes = [c_void_p, c_int, c_int, c_int, c_int]
        L.vp8hip_geometry.argtypes = [c_void_p, c_void_p]
        L.vp8hip_ir_map.argtypes = [c_void_p, c_int] + [ctypes.POINTER(c_void_p)] * 4
        L.vp8hip_ir_upload.argtypes = [c_void_p, c_int]
        L.vp8hip_ir_map_compact.argtypes = [c_void_p, c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p),
                                            ctypes.POINTER(c_size_t), ctypes.POINTER(c_void_p)]
        L.vp8hip_ir_upload_compact.argtypes = [c_void_p, c_int, c_size_t]
        L.vp8hip_ir_copy.argtypes = [c_void_p, c_int, c_int]
        L.vp8hip_decode.argtypes = [c_void_p, c_void_p, c_int, c_int]
        L.vp8hip_frame_download.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int]
        L.vp8hip_frame_upload.argtypes = [c_void_p, c_int, c_void_p]
        L.vp8hip_frame_copy.argtypes = [c_void_p, c_int, c_int]
        L.vp8hip_frames_to_raster.argtypes = [c_void_p, c_int, c_int]
        L.vp8hip_set_direct_download.argtypes = [c_void_p, c_int]
        L.vp8hip_set_pred_tiles.argtypes = [c_void_p, c_int]
        L.vp8hip_sync.argtypes = [c_void_p]
        L.vp8hip_join.argtypes = [c_void_p]
        L.vp8hip_get_stats_at.argtypes = [c_void_p, c_int, ctypes.POINTER(Stats)]
        L.vp8hip_get_stats.argtypes = [c_void_p, c_void_p]
        L.vp8hip_stream.argtypes = [c_void_p]
        L.vp8hip_stream.restype = c_void_p
        L.vp8hip_postproc.argtypes = [c_void_p, c_int, c_int, c_int, ctypes.POINTER(PostprocParams)]
        L.vp8hip_mfqe.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int]
        L.vp8hip_visualize.argtypes = [c_void_p, c_int, c_int, ctypes.POINTER(VisParams)]
        L.vp8hip_entropy_decode.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t]
        L.vp8hip_entropy_status.argtypes = [c_void_p, c_int, c_void_p]
        L.vp8hip_ir_fetch.argtypes = [c_void_p, c_int, c_void_p, c_void_p]
        L.vp8hip_ir_fetch_mvs.argtypes = [c_void_p, c_int, c_void_p]
        L.vp8hip_i420_size.argtypes = [c_int, c_int]
        L.vp8hip_i420_size.restype = c_size_t
        L.vp8hip_frames_scale_async.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t]
        L.vp8hip_device.argtypes = [c_void_p]
        L.vp8hip_rgb_size.argtypes = [ctypes.POINTER(RgbParams)]
        L.vp8hip_rgb_size.restype = c_size_t
        L.vp8hip_frames_rgb_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(RgbParams), c_void_p, c_size_t]
        L.vp8hip_rgb_scratch_bytes.argtypes = [c_void_p]
        L.vp8hip_rgb_scratch_bytes.restype = c_size_t
        L.vp8hip_release_staging.argtypes = [c_void_p]
        L.vp8hip_side_mv_size.argtypes = [c_void_p, ctypes.POINTER(SideParams)]
        L.vp8hip_side_mv_size.restype = c_size_t
        L.vp8hip_side_info_size.argtypes = [c_void_p, ctypes.POINTER(SideParams)]
        L.vp8hip_side_info_size.restype = c_size_t
        L.vp8hip_frames_side_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(SideParams), c_void_p, c_size_t, c_void_p, c_size_t]
        L.vp8hip_residual_size.argtypes = [c_void_p, ctypes.POINTER(ResidualParams)]
        L.vp8hip_residual_size.restype = c_size_t
        L.vp8hip_frames_residual_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(ResidualParams), c_void_p, c_size_t]
        L.vp8hip_coef_size.argtypes = [c_void_p, ctypes.POINTER(CoefParams)]
        L.vp8hip_coef_size.restype = c_size_t
        L.vp8hip_frames_coef_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(CoefParams), c_void_p, c_size_t]
        L.vp8hip_dequant_factors.argtypes = [c_void_p, c_void_p]
        L.vp8hip_trace_size.argtypes = [c_void_p]
        L.vp8hip_trace_size.restype = c_size_t
        L.vp8hip_frames_trace_async.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_int]
        L.vp8hip_trace_flow_size.argtypes = [c_void_p, ctypes.POINTER(TraceFlowParams)]
        L.vp8hip_trace_flow_size.restype = c_size_t
        L.vp8hip_trace_flow_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(TraceFlowParams), c_void_p, c_size_t, c_int, c_void_p,
                                              c_size_t]
        L.vp8hip_trace_residual_size.argtypes = [c_void_p, ctypes.POINTER(TraceResidualParams)]
        L.vp8hip_trace_residual_size.restype = c_size_t
        L.vp8hip_trace_residual_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(TraceResidualParams), c_void_p, c_size_t, c_int,
                                                  c_void_p, c_size_t]
        L.vp8hip_trace_gather_size.argtypes = [c_void_p, ctypes.POINTER(TraceGatherParams)]
        L.vp8hip_trace_gather_size.restype = c_size_t
        L.vp8hip_trace_gather_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(TraceGatherParams), c_void_p, c_size_t, c_int,
                                                c_void_p, c_size_t, c_int, c_void_p, c_size_t]
        L.vp8hip_frames_wear_async.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_int]
        L.vp8hip_trace_wear_size.argtypes = [c_void_p, ctypes.POINTER(TraceWearParams)]
        L.vp8hip_trace_wear_size.restype = c_size_t
        L.vp8hip_trace_wear_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(TraceWearParams), c_void_p, c_size_t, c_int, c_void_p,
                                              c_size_t]
        L.vp8hip_trace_invert_async.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_void_p, c_size_t,
                                                c_int]
        L.vp8hip_trace_cover_size.argtypes = [c_void_p, ctypes.POINTER(TraceCoverParams)]
        L.vp8hip_trace_cover_size.restype = c_size_t
        L.vp8hip_trace_cover_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(TraceCoverParams), c_void_p, c_size_t, c_int, c_void_p,
                                               c_size_t]
        L.vp8hip_hist_size.argtypes = [c_int]
        L.vp8hip_hist_size.restype = c_size_t
        L.vp8hip_frames_hist_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_uint, c_void_p, c_size_t]
        L.vp8hip_slots_hist_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_uint, c_void_p, c_size_t]
        L.vp8hip_trace_wear_hist_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_uint, c_void_p, c_size_t, c_int, c_void_p, c_size_t]
        L.vp8hip_trace_cover_hist_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_uint, c_void_p, c_size_t, c_int, c_void_p, c_size_t]
        L.vp8hip_ssim_windows.argtypes = [c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
        L.vp8hip_ssim_scores_size.argtypes = [c_int]
        L.vp8hip_ssim_scores_size.restype = c_size_t
        L.vp8hip_ssim_map_size.argtypes = [c_void_p, ctypes.POINTER(SsimParams)]
        L.vp8hip_ssim_map_size.restype = c_size_t
        L.vp8hip_ssim_share.argtypes = [c_void_p, c_int, ctypes.c_uint]
        L.vp8hip_frames_ssim_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(SsimParams), c_void_p, c_size_t, c_void_p, c_size_t]
        L.vp8hip_motion_mv_size.argtypes = [c_void_p]
        L.vp8hip_motion_mv_size.restype = c_size_t
        L.vp8hip_motion_stats_size.argtypes = [c_void_p, ctypes.POINTER(MotionParams)]
        L.vp8hip_motion_stats_size.restype = c_size_t
        L.vp8hip_frames_motion_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(MotionParams), c_void_p, c_size_t, c_void_p, c_size_t,
                                                 c_void_p, c_size_t]
        L.vp8hip_subpel_mv_size.argtypes = [c_void_p]
        L.vp8hip_subpel_mv_size.restype = c_size_t
        L.vp8hip_subpel_stats_size.argtypes = [c_void_p, ctypes.POINTER(SubpelParams)]
        L.vp8hip_subpel_stats_size.restype = c_size_t
        L.vp8hip_frames_subpel_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(SubpelParams), c_void_p, c_size_t, c_void_p, c_size_t,
                                                 c_void_p, c_size_t, c_void_p, c_size_t]
        L.vp8hip_tfilter_count_size.argtypes = [c_void_p]
        L.vp8hip_tfilter_count_size.restype = c_size_t
        L.vp8hip_frames_tfilter_async.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_int, ctypes.POINTER(TfilterParams), c_void_p, c_size_t,
                                                  c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t]
        L.vp8hip_quant_factors.argtypes = [c_int, c_void_p, c_void_p]
        for name in ("vp8hip_quant_coef_size", "vp8hip_quant_eob_size"):
            getattr(L, name).argtypes = [c_void_p]
            getattr(L, name).restype = c_size_t
        L.vp8hip_quant_stats_size.argtypes = [c_void_p, ctypes.POINTER(QuantParams)]
        L.vp8hip_quant_stats_size.restype = c_size_t
        L.vp8hip_frames_quant_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(QuantParams), c_void_p, c_size_t, c_void_p, c_size_t,
                                                c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t]
        L.vp8hip_intra_costs.argtypes = [ctypes.POINTER(IntraCost)]
        L.vp8hip_intra_rd.argtypes = [c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
        L.vp8hip_intra_modes_size.argtypes = [c_void_p]
        L.vp8hip_intra_modes_size.restype = c_size_t
        L.vp8hip_intra_stats_size.argtypes = [c_void_p, ctypes.POINTER(IntraParams)]
        L.vp8hip_intra_stats_size.restype = c_size_t
        L.vp8hip_frames_intra_async.argtypes = [c_void_p, c_void_p, c_int, ctypes.POINTER(IntraParams), c_void_p, c_size_t, c_void_p, c_size_t,
                                                c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t]
        L.vp8hip_pack_bound.argtypes = [c_void_p, c_int]
        L.vp8hip_pack_bound.restype = c_size_t
        L.vp8hip_pack_header.argtypes = [ctypes.POINTER(PackParams), c_int, ctypes.POINTER(PackHead)]
        L.vp8hip_frames_pack_async.argtypes = [c_void_p, c_int, ctypes.POINTER(PackParams), c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t,
                                               c_size_t, c_void_p]
        L.vp8hip_pack_adapt_bound.argtypes = [c_void_p, c_int]
        L.vp8hip_pack_adapt_bound.restype = c_size_t
        L.vp8hip_pack_probs_default.argtypes = [c_void_p]
        L.vp8hip_pack_probs_default.restype = None
        L.vp8hip_pack_header_prefix.argtypes = [ctypes.POINTER(PackParams), c_int, c_int, ctypes.POINTER(PackHead)]
        L.vp8hip_frames_pack_adapt_async.argtypes = [c_void_p, c_int, ctypes.POINTER(PackParams), ctypes.POINTER(PackAdapt), c_void_p, c_size_t, c_void_p,
                                                     c_size_t, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p]
        L.vp8hip_pack_key_bound.argtypes = [c_void_p, c_int]
        L.vp8hip_pack_key_bound.restype = c_size_t
        L.vp8hip_pack_key_header.argtypes = [ctypes.POINTER(PackKeyParams), c_int, ctypes.POINTER(PackHead)]
        L.vp8hip_frames_pack_key_async.argtypes = [c_void_p, c_int, ctypes.POINTER(PackKeyParams), c_void_p, c_size_t, c_void_p, c_size_t, c_void_p,
                                                   c_size_t, c_size_t, c_void_p]
        # One HIP runtime per process: torch carries its own libamdhip64 (SONAME libamdhip64.so.7), which libvp8hip.so's
        # dependency resolves to only if torch was loaded first; otherwise torch maps a second runtime later, whose device
        # pointers this library's runtime does not know
        global _torch_first
        _torch_first = "torch" in sys.modules
        _hip = L
    return _hip


class Vp8Hip:
    """One HIP context = one GPU's frame-buffer pool + IR slots + stream."""

    def __init__(self, device=-1):
        self.L = load_hip()
        h = c_void_p()
        if self.L.vp8hip_create(device, ctypes.byref(h)):
            raise RuntimeError("vp8hip_create: " + self.L.vp8hip_last_error(None).decode())
        self.h = h
        self.width = self.height = 0
        self.g = None

    def _chk(self, rc, what):
        if rc:
            raise RuntimeError(f"{what}: {self.L.vp8hip_last_error(self.h).decode()}")

    def close(self):
        if self.h:
            self.L.vp8hip_destroy(self.h)
            self.h = None

    def configure(self, width, height, num_fb, num_slots):
        self._chk(self.L.vp8hip_configure(self.h, width, height, num_fb, num_slots), "vp8hip_configure")
        self.width, self.height = width, height
        self.g = geom(width, height)
        self.nmb = (self.g.aligned_w // 16) * (self.g.aligned_h // 16)
        self.num_fb, self.num_slots = num_fb, num_slots

    def configure_pooled(self, width, height, num_fb, num_slots, pool_bytes):
        """vp8hip_configure_pooled: slots without block streams of their own + one pool the device's entropy decoder fills"""
        self.L.vp8hip_configure_pooled.argtypes = [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t]
        self._chk(self.L.vp8hip_configure_pooled(self.h, width, height, num_fb, num_slots, pool_bytes), "vp8hip_configure_pooled")
        self.width, self.height = width, height
        self.g = geom(width, height)
        self.nmb = (self.g.aligned_w // 16) * (self.g.aligned_h // 16)
        self.num_fb, self.num_slots = num_fb, num_slots

    def memory_usage(self):
        """vp8hip_memory_usage -> dict of bytes the context holds on the device: raster_pool, tile_pool, slots, block_pool,
        entropy_input, packed_staging"""
        out = (ctypes.c_size_t * 6)()
        self.L.vp8hip_memory_usage.argtypes = [c_void_p, c_void_p]
        self._chk(self.L.vp8hip_memory_usage(self.h, out), "vp8hip_memory_usage")
        return dict(zip(("raster_pool", "tile_pool", "slots", "block_pool", "entropy_input", "packed_staging"), [int(v) for v in out]))

    def pool_reset(self):
        self.L.vp8hip_pool_reset.argtypes = [c_void_p]
        self._chk(self.L.vp8hip_pool_reset(self.h), "vp8hip_pool_reset")

    def pool_usage(self):
        """-> (bytes taken since the last reset, bytes the pool holds)"""
        used, size = ctypes.c_size_t(), ctypes.c_size_t()
        self.L.vp8hip_pool_usage.argtypes = [c_void_p, c_void_p, c_void_p]
        self._chk(self.L.vp8hip_pool_usage(self.h, ctypes.byref(used), ctypes.byref(size)), "vp8hip_pool_usage")
        return used.value, size.value

    def ir_map(self, slot):
        ptrs = [c_void_p() for _ in range(4)]
        self._chk(self.L.vp8hip_ir_map(self.h, slot, *[ctypes.byref(p) for p in ptrs]), "vp8hip_ir_map")
        return [p.value for p in ptrs]   # hdr, mbs, coef, mvs (pinned host addresses)

    def fill_slot(self, slot, hdr, mbs, coef, mvs):
        """Copy numpy IR arrays into a slot's pinned staging and upload it."""
        ph, pm, pc, pv = self.ir_map(slot)
        ctypes.memmove(ph, ctypes.byref(hdr), 64)
        ctypes.memmove(pm, mbs.ctypes.data, mbs.nbytes)
        ctypes.memmove(pc, coef.ctypes.data, coef.nbytes)
        if hdr.frame_type != 0:
            ctypes.memmove(pv, mvs.ctypes.data, mvs.nbytes)
        self.upload(slot)

    def parse_into_slot(self, parser, data, slot):
        """Feeder writes straight into the pinned staging of `slot`; returns hdr (not yet uploaded)."""
        hdr, changed = parser.begin(data)
        if (hdr.width, hdr.height) != (self.width, self.height):
            parser.abandon()             # (so that the same call on the same parser works once the context is configured)
            raise RuntimeError("dimension change: reconfigure the context first")
        ph, pm, pc, pv = self.ir_map(slot)
        parser.decode_mbs(pm, pc, pv)
        ctypes.memmove(ph, ctypes.byref(hdr), 64)
        return hdr

    def ir_map_compact(self, slot):
        """Pinned staging of `slot` in the device form: (hdr, mbx, blocks, mvs addresses, blocks the stream may take)."""
        ph, pm, pb, pv, cap = c_void_p(), c_void_p(), c_void_p(), c_void_p(), c_size_t()
        self._chk(self.L.vp8hip_ir_map_compact(self.h, slot, ctypes.byref(ph), ctypes.byref(pm), ctypes.byref(pb), ctypes.byref(cap),
                                               ctypes.byref(pv)), "vp8hip_ir_map_compact")
        return ph.value, pm.value, pb.value, pv.value, cap.value

    def parse_into_slot_compact(self, parser, data, slot):
        """Feeder writes the frame in the DEVICE FORM (include/vp8_ir.h) into the pinned staging of `slot` and queues the upload
        (one copy; nothing on the device touches the slot before the pixel kernels read it); returns (hdr, bytes uploaded)."""
        hdr, changed = parser.begin(data)
        if (hdr.width, hdr.height) != (self.width, self.height):
            parser.abandon()             # (so that the same call on the same parser works once the context is configured)
            raise RuntimeError("dimension change: reconfigure the context first")
        ph, pm, pb, pv, cap = self.ir_map_compact(slot)
        nb, _ = parser.decode_mbs_compact(pm, pb, cap, pv)
        parser.final_hdr(hdr)
        ctypes.memmove(ph, ctypes.byref(hdr), 64)
        self._chk(self.L.vp8hip_ir_upload_compact(self.h, slot, nb), "vp8hip_ir_upload_compact")
        return hdr, self.nmb * 128 + nb * 32

    def fill_slot_compact(self, slot, hdr, mbx, blocks, mvs):
        """numpy arrays in the device form (compact_from_dense) into a slot's pinned staging, and up."""
        ph, pm, pb, pv, cap = self.ir_map_compact(slot)
        assert blocks.shape[0] <= cap
        ctypes.memmove(ph, ctypes.byref(hdr), 64)
        ctypes.memmove(pm, mbx.ctypes.data, mbx.nbytes)
        if blocks.nbytes:
            ctypes.memmove(pb, blocks.ctypes.data, blocks.nbytes)
        if hdr.frame_type != 0:
            ctypes.memmove(pv, mvs.ctypes.data, mvs.nbytes)
        self._chk(self.L.vp8hip_ir_upload_compact(self.h, slot, blocks.shape[0]), "vp8hip_ir_upload_compact")

    def upload(self, slot):
        self._chk(self.L.vp8hip_ir_upload(self.h, slot), "vp8hip_ir_upload")

    def ir_copy(self, dst, src):
        self._chk(self.L.vp8hip_ir_copy(self.h, dst, src), "vp8hip_ir_copy")

    @staticmethod
    def job_array(jobs):
        """list of (ir_slot, dst_fb, (last, golden, alt) or None) -> a vp8hip_job array (for decode_array, or frames_trace as it is)"""
        arr = (Job * max(len(jobs), 1))()
        for i, (slot, dst, refs) in enumerate(jobs):
            arr[i].ir_slot, arr[i].dst_fb = slot, dst
            arr[i].ref_fb[0] = -1
            for k in range(3):
                arr[i].ref_fb[k + 1] = refs[k] if refs is not None else -1
        return arr

    def decode(self, jobs, stages=STAGE_ALL):
        """jobs: list of (ir_slot, dst_fb, (last, golden, alt))"""
        arr = self.job_array(jobs)
        self._jobs_keepalive = arr
        self._chk(self.L.vp8hip_decode(self.h, arr, len(jobs), stages), "vp8hip_decode")

    def decode_array(self, job_array, n, stages=STAGE_ALL):
        self._chk(self.L.vp8hip_decode(self.h, job_array, n, stages), "vp8hip_decode")

    def sync(self):
        self._chk(self.L.vp8hip_sync(self.h), "vp8hip_sync")

    def join(self):
        """Order the context's main stream behind a tiled->raster pass still running on the internal stream."""
        self._chk(self.L.vp8hip_join(self.h), "vp8hip_join")

    def stats(self, back=0):
        """Kernel times of the last launch (back=0) or of an earlier one (back <= 31); waits for that launch only."""
        s = Stats()
        self._chk(self.L.vp8hip_get_stats_at(self.h, back, ctypes.byref(s)), "vp8hip_get_stats_at")
        return s

    def stream(self):
        return self.L.vp8hip_stream(self.h)

    def download_full(self, fb):
        buf = np.empty(self.g.frame_size, np.uint8)
        self._chk(self.L.vp8hip_frame_download(self.h, fb, 1, buf.ctypes.data, None, None, 0, 0), "download")
        return buf

    def download_planes(self, fb):
        w, h = self.width, self.height
        cw, ch = (w + 1) // 2, (h + 1) // 2
        y, u, v = np.empty((h, w), np.uint8), np.empty((ch, cw), np.uint8), np.empty((ch, cw), np.uint8)
        self._chk(self.L.vp8hip_frame_download(self.h, fb, 0, y.ctypes.data, u.ctypes.data, v.ctypes.data, w, cw),
                  "download")
        return y, u, v

    def frames_md5(self, first_fb, count):
        """MD5s of `count` consecutive frame buffers computed on the device (vp8hip_frames_fetch_async): list of hex digests."""
        out = np.zeros(16 * count, np.uint8)
        self.L.vp8hip_frames_fetch_async.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        self.L.vp8hip_download_wait.argtypes = [ctypes.c_void_p]
        self._chk(self.L.vp8hip_frames_fetch_async(self.h, first_fb, count, None, out.ctypes.data), "vp8hip_frames_fetch_async")
        self._chk(self.L.vp8hip_download_wait(self.h), "vp8hip_download_wait")
        return [out[16 * i: 16 * i + 16].tobytes().hex() for i in range(count)]

    def frames_i420(self, first_fb, count):
        """`count` consecutive frame buffers as packed I420 (vp8hip_frames_fetch_i420_async: packed on the device from whichever form
        they are in -- tiles as they are --, no raster pool needed): uint8 array [count, w * h + 2 * (w / 2) * ((h + 1) / 2)]."""
        self.L.vp8hip_i420_bytes.restype = ctypes.c_size_t
        self.L.vp8hip_i420_bytes.argtypes = [ctypes.c_void_p]
        self.L.vp8hip_frames_fetch_i420_async.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        self.L.vp8hip_download_wait.argtypes = [ctypes.c_void_p]
        nb = self.L.vp8hip_i420_bytes(self.h)
        # (the destination of a batch fetch is page-locked memory, include/vp8hip.h: into pageable memory the asynchronous copies of
        # the fetch's streams would be staged by the runtime one after the other)
        self.L.vp8hip_host_alloc.restype = ctypes.c_void_p
        self.L.vp8hip_host_alloc.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        self.L.vp8hip_host_free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        host = self.L.vp8hip_host_alloc(self.h, nb * count)
        if not host:
            raise RuntimeError("vp8hip_host_alloc: " + self.L.vp8hip_last_error(self.h).decode())
        try:
            self._chk(self.L.vp8hip_frames_fetch_i420_async(self.h, first_fb, count, host, None), "vp8hip_frames_fetch_i420_async")
            self._chk(self.L.vp8hip_download_wait(self.h), "vp8hip_download_wait")
            out = np.ctypeslib.as_array(ctypes.cast(host, ctypes.POINTER(ctypes.c_uint8)), shape=(count, nb)).copy()
        finally:
            self.L.vp8hip_host_free(self.h, host)
        return out

    def device(self):
        """the HIP device index the context runs on (-1 at creation resolved)"""
        return self.L.vp8hip_device(self.h)

    def frames_scaled(self, fbs, width=None, height=None, filter=1, out=None):
        """Frame buffers `fbs` (any order, repeats allowed) as packed I420 on the context's device, at the display size (a copy) or
        scaled to width x height as libyuv's I420Scale scales them (vp8hip_frames_scale_async; filter 0 point, 1 bilinear, 2 = 1):
        a torch.uint8 tensor [n, i420_size(width, height)] -- `out` when given (a view is fine: stride(1) == 1, stride(0) is the
        frame stride).  Ordered against torch's current stream both ways: usable there without a sync, and the tensor may outlive
        the context.  The tensor is not recorded on the context's stream (record_stream would make freeing it after close() touch a
        destroyed stream): an `out` allocated on another stream than the current one must not be freed and reused on that stream
        before torch's current stream has passed this call.  split_i420 gives the planes."""
        fbs = [int(f) for f in fbs]
        w = self.width if width is None else int(width)
        h = self.height if height is None else int(height)
        size = int(self.L.vp8hip_i420_size(w, h))

        def ok(out, dtype, shape, dev):
            return out.dtype == dtype and out.dim() == 2 and out.shape[0] == len(fbs) and out.shape[1] == size and out.stride(1) == 1 \
                and out.device == dev
        return self._to_torch("frames_scaled", [("out", out, "uint8", (len(fbs), size))],
                              lambda arr_out, stride: self.L.vp8hip_frames_scale_async(
                                  self.h, (c_int * max(len(fbs), 1))(*fbs), len(fbs), w, h, int(filter), arr_out, stride),
                              "vp8hip_frames_scale_async", ok, "with stride(1) == 1")[0]

    @staticmethod
    def _dense(t, dtype, shape, dev):
        """t is a tensor of this type and shape [n, ...] on this device, each frame dense (stride(0) free)"""
        return t.dtype == dtype and tuple(t.shape) == tuple(shape) and (shape[0] == 0 or t[0].is_contiguous()) and t.device == dev

    def _to_torch(self, who, outs, call, what, ok=None, how="each frame dense"):
        """The torch side of a hand-over on the device (frames_scaled, frames_rgb, frames_side, frames_residual).  outs: one or two
        of (the argument's name, the caller's tensor or None, the type's name, the shape [n, ...]); a tensor is made here when
        None and checked otherwise (ok: _dense).  Then call(data pointer, frame stride in bytes -- and the same of the second
        tensor) between the two stream waits.  Returns the tensors."""
        torch, dev = self._torch_device(who)
        made = []
        for arg, out, name, shape in outs:
            if out is None:
                out = torch.empty(tuple(shape), dtype=getattr(torch, name), device=dev)
            if not (ok or self._dense)(out, getattr(torch, name), shape, dev):
                raise ValueError(f"{who}: {arg} must be a {name} tensor {list(shape)}, {how}, on {dev}")
            made.append(out)
        args = [a for t in made for a in (c_void_p(t.data_ptr()), t.stride(0) * t.element_size())]
        self._between_stream_waits(dev, lambda: call(*args), what)
        return made

    def _grid(self, who, width, height, cells):
        """-> (native, gw, gh): the output grid of width x height, or with neither the native one, `cells` a macroblock each way"""
        native = width is None and height is None
        if not native and (width is None or height is None):
            raise ValueError(f"{who}: width and height, or neither")
        if native:
            return True, cells * (self.g.aligned_w // 16), cells * (self.g.aligned_h // 16)
        return False, int(width), int(height)

    def _trace_grid(self, who, width, height):
        """-> (dst_w, dst_h, gw, gh) of a call that reads a trace pool; with no size 0, 0 and the display size, the trace's own grid"""
        native, gw, gh = self._grid(who, width, height, 16)
        return (0, 0, self.width, self.height) if native else (gw, gh, gw, gh)

    @staticmethod
    def _trace_jobs(who, jobs, struct, fields):
        """-> (the jobs of a call that reads a trace pool, tuples of ints, as an array of `struct`; how many)"""
        jobs = [tuple(int(v) for v in j) for j in jobs]
        if any(len(j) != len(struct._fields_) for j in jobs):
            raise ValueError(f"{who}: jobs are {fields}")
        return (struct * max(len(jobs), 1))(*jobs), len(jobs)

    def _torch_device(self, who):
        """-> (torch, the context's device as torch names it); refuses when torch came after the library"""
        import torch
        if not _torch_first:
            raise RuntimeError(f"{who}: import torch before the first Vp8Hip (one HIP runtime per process: torch loaded after "
                               "libvp8hip.so maps a second one, whose device pointers this library cannot use)")
        return torch, torch.device("cuda", self.device())

    def _between_stream_waits(self, dev, fn, what):
        """fn() -- a call that writes torch tensors on the context's stream; its status is checked as `what` -- ordered against
        torch's current stream both ways"""
        import torch
        ext = torch.cuda.ExternalStream(self.stream(), device=dev)
        cur = torch.cuda.current_stream(dev)
        ext.wait_stream(cur)                    # whatever torch queued that touches the tensors first
        self._chk(fn(), what)
        cur.wait_stream(ext)                    # torch's work after this call sees what was written
        # (no record_stream(ext) on the tensors: the allocator would record an event on the context's stream when one is freed,
        # which crashes once the context -- and its stream -- is gone; torch's stream waiting on ours already orders any reuse)

    def frames_rgb(self, fbs, width=None, height=None, filter=1, dtype=None, layout="nchw", order="rgb", matrix="bt601", mean=None, std=None,
                   out=None):
        """Frame buffers `fbs` (any order, repeats allowed) as RGB on the context's device (vp8hip_frames_rgb_async): a tensor
        [n, 3, h, w] ("nchw"), [n, h, w, 3] ("nhwc") or [n, h, w, 4] ("nhwc4": fourth byte 255, uint8 only) of torch.uint8 (the
        default), torch.float16 or torch.float32, channels in `order` ("rgb" / "bgr"), at the display size or scaled as
        frames_scaled scales (width, height, filter), converted with `matrix` ("bt601": limited range, what a VP8 stream is;
        "bt601-full"; "bt709"): the integer arithmetic of include/vp8hip.h, chroma replicated.  Float types: the value for byte v
        of colour c (R, G, B) is float32(float64(v) * scale[c] + bias[c]) -- float16: that, rounded to nearest-even -- with
        scale = float32(1 / (255 * std)) and bias = float32(-mean / std), each computed in float64 from `mean` / `std` (per colour,
        on the 0..1 scale; default 0 and 1) and cast once: THIS PAIR of float32 numbers defines the values, not (v / 255 - mean) /
        std evaluated some other way.  `out`: the inner three dimensions dense, stride(0) free.  Stream ordering, the `import
        torch` first rule and the remark on record_stream: as frames_scaled."""
        import torch
        fbs = [int(f) for f in fbs]
        w = self.width if width is None else int(width)
        h = self.height if height is None else int(height)
        dtype = torch.uint8 if dtype is None else dtype
        dt = _elem_dtype(dtype, _RGB_DTYPES)
        if dt is None or layout not in RGB_LAYOUTS or order not in RGB_ORDERS or matrix not in RGB_MATRICES:
            raise ValueError(f"frames_rgb: dtype {dtype}, layout {layout!r}, order {order!r}, matrix {matrix!r}")
        mean = np.zeros(3) if mean is None else np.asarray(mean, np.float64).reshape(3)
        std = np.ones(3) if std is None else np.asarray(std, np.float64).reshape(3)
        p = RgbParams(w, h, int(filter), RGB_MATRICES[matrix], RGB_LAYOUTS[layout], RGB_ORDERS[order], dt)
        for c in range(3):
            p.scale[c] = np.float32(1.0 / (255.0 * std[c]))
            p.bias[c] = np.float32(-mean[c] / std[c])
        if not self.L.vp8hip_rgb_size(ctypes.byref(p)):
            raise ValueError(f"frames_rgb: {w}x{h}, filter {filter}, {dtype}, layout {layout!r}: refused (sizes 1..16383; nhwc4 is uint8 only)")
        shape = (3, h, w) if layout == "nchw" else (h, w, 3 if layout == "nhwc" else 4)
        return self._to_torch("frames_rgb", [("out", out, _RGB_DTYPES[dt], (len(fbs),) + shape)],
                              lambda arr_out, stride: self.L.vp8hip_frames_rgb_async(
                                  self.h, (c_int * max(len(fbs), 1))(*fbs), len(fbs), ctypes.byref(p), arr_out, stride),
                              "vp8hip_frames_rgb_async")[0]

    def frames_side(self, slots, width=None, height=None, mv_dtype=None, planes=("ref", "mode", "skip"), scale=None, out_mv=None,
                    out_info=None):
        """IR slots `slots` (any order, repeats allowed) as (mv, info) tensors on the context's device (vp8hip_frames_side_async):
        mv [n, 2, gh, gw] of torch.int16 (the default: the stored 1/8-pel vectors), torch.float16 or torch.float32, channel 0 = x,
        1 = y; info [n, C, gh, gw] of torch.uint8, the planes of `planes` ("ref", "mode", "skip", "segment", "qindex", "coded", or
        the mask) in bit order.  With no size the native grid, a cell per 4x4 luma block of the coded area (gw, gh = 4 * mb_cols,
        4 * mb_rows); with width x height the cell under each output pixel's centre (include/vp8hip.h), so that at frames_rgb's
        size the tensors line up with its pixels.  Float types: float32(float64(v) * scale[c]) with scale = (x, y) float32 numbers
        (default 1, 1); scale="pixels" is (0.125 * gw / d_w, 0.125 * gh / d_h), computed in float64 and rounded once: the flow in
        pixels of the tensor (native grid: d_w, d_h = the coded size).  planes=() gives info None, and out_mv=False / out_info=False
        skip that tensor; a tensor passed as out_mv / out_info is filled (each frame dense, stride(0) free).  Stream ordering, the
        `import torch` first rule and the remark on record_stream: as frames_scaled."""
        torch = self._torch_device("frames_side")[0]
        slots = [int(s) for s in slots]
        n = len(slots)
        native, gw, gh = self._grid("frames_side", width, height, 4)
        mv_dtype = torch.int16 if mv_dtype is None else mv_dtype
        dt, mask = _elem_dtype(mv_dtype, _INT16_DTYPES), _plane_mask(planes, SIDE_PLANES, True)
        if dt is None or mask is None:
            raise ValueError(f"frames_side: mv_dtype {mv_dtype}, planes {planes!r}")
        want_mv = out_mv is not False
        want_info = out_info is not False and mask != 0
        if not want_mv and not want_info:
            raise ValueError("frames_side: neither tensor asked for")
        if scale is None:
            sc = (1.0, 1.0)
        elif isinstance(scale, str):
            if scale != "pixels":
                raise ValueError(f"frames_side: scale {scale!r}")
            dw, dh = (self.g.aligned_w, self.g.aligned_h) if native else (self.width, self.height)
            sc = (0.125 * gw / dw, 0.125 * gh / dh)
        else:
            sc = tuple(float(v) for v in scale)
        p = SideParams(0 if native else gw, 0 if native else gh, dt, mask)
        p.scale[0], p.scale[1] = np.float32(sc[0]), np.float32(sc[1])
        if not self.L.vp8hip_side_mv_size(self.h, ctypes.byref(p)):
            raise ValueError(f"frames_side: grid {gw}x{gh}: refused (sizes 1..16383)")
        nc = bin(mask).count("1")
        outs = [("out_mv", out_mv, _INT16_DTYPES[dt], (n, 2, gh, gw))] if want_mv else []
        if want_info:
            outs.append(("out_info", out_info, "uint8", (n, nc, gh, gw)))
        none = (None, 0)

        def call(*args):        # (pointer and stride of each tensor asked for)
            mv, info = (args[:2] if want_mv else none), (args[-2:] if want_info else none)
            return self.L.vp8hip_frames_side_async(self.h, (c_int * max(n, 1))(*slots), n, ctypes.byref(p), *mv, *info)
        made = self._to_torch("frames_side", outs, call, "vp8hip_frames_side_async")
        return made[0] if want_mv else None, made[-1] if want_info else None

    def frames_residual(self, slots, width=None, height=None, dtype=None, layout="planar", scale=None, out=None):
        """IR slots `slots` (any order, repeats allowed) as residual tensors on the context's device
        (vp8hip_frames_residual_async): what the stream adds to the prediction, before the clamp, as include/vp8hip.h defines
        it.  layout "planar": [n, 3, gh, gw], chroma replicated, sample for sample frames_rgb's "nchw" tensor at that size;
        "i420": a flat [n, elements], the three planes at their own sizes (split_residual gives the views).  torch.int16 (the
        default), torch.float16 or torch.float32; float types: float32(float64(v) * scale[c]) with scale = one number or (Y, U,
        V), float32 (default 1).  With no size the native grid: the coded area, gw, gh = 16 * mb_cols, 16 * mb_rows; with width
        x height the sample under each output's centre, at the display size a crop.  `out`: a tensor of that shape and type,
        each frame dense, stride(0) free.  Stream ordering, the `import torch` first rule and the remark on record_stream: as
        frames_scaled."""
        import torch
        slots = [int(s) for s in slots]
        n = len(slots)
        native, gw, gh = self._grid("frames_residual", width, height, 16)
        dtype = torch.int16 if dtype is None else dtype
        dt = _elem_dtype(dtype, _INT16_DTYPES)
        if dt is None or layout not in RES_LAYOUTS:
            raise ValueError(f"frames_residual: dtype {dtype}, layout {layout!r}")
        if scale is None:
            sc = (1.0, 1.0, 1.0)
        elif np.ndim(scale) == 0:
            sc = (float(scale),) * 3
        else:
            sc = tuple(float(v) for v in scale)
            if len(sc) != 3:
                raise ValueError(f"frames_residual: scale {scale!r}")
        p = ResidualParams(0 if native else gw, 0 if native else gh, RES_LAYOUTS[layout], dt)
        for c in range(3):
            p.scale[c] = np.float32(sc[c])
        size = int(self.L.vp8hip_residual_size(self.h, ctypes.byref(p)))
        if not size:
            raise ValueError(f"frames_residual: grid {gw}x{gh}: refused (sizes 1..16383)")
        shape = (3, gh, gw) if layout == "planar" else (size // (2, 2, 4)[dt],)
        return self._to_torch("frames_residual", [("out", out, _INT16_DTYPES[dt], (n,) + shape)],
                              lambda arr_out, stride: self.L.vp8hip_frames_residual_async(
                                  self.h, (c_int * max(n, 1))(*slots), n, ctypes.byref(p), arr_out, stride),
                              "vp8hip_frames_residual_async")[0]

    def frames_coef(self, slots, stage="dequant", layout="channels", planes=("y", "u", "v"), nfreq=16, order="raster", dtype=None, scale=None,
                    out=None):
        """IR slots `slots` (any order, repeats allowed) as transform-coefficient tensors on the context's device
        (vp8hip_frames_coef_async; include/vp8hip.h has the definition): stage "levels", what the stream codes, or "dequant", the
        values that enter the inverse transforms.  -> {plane: view} for the planes of `planes` ("y", "u", "v", "y2", or the mask), views
        into ONE tensor [n, elements] that holds them back to back in bit order (split_coef): layout "channels" [n, nfreq, G * mb_rows,
        G * mb_cols] with G = 4, 2, 2, 1 blocks of a macroblock each way, channel j position j = 4 * v + u of the block (order "raster")
        or position COEF_ZIGZAG[j] ("zigzag"), the first nfreq of them; "inplace" [n, 4 * G * mb_rows, 4 * G * mb_cols], the residual's
        geometry (nfreq 16, "raster").  The coded area only: coefficients are not resampled.  torch.int16 (the default), torch.float16
        or torch.float32; float types: float32(float64(v) * scale[plane]) with scale = one number or one per plane of (Y, U, V, Y2),
        float32 (default 1).  `out`: the [n, elements] tensor to fill, each frame dense, stride(0) free.  Stream ordering, the `import
        torch` first rule and the remark on record_stream: as frames_scaled."""
        import torch
        slots = [int(s) for s in slots]
        n = len(slots)
        dtype = torch.int16 if dtype is None else dtype
        made = _coef_params(stage, layout, planes, nfreq, order, dtype)
        if made is None:
            raise ValueError(f"frames_coef: stage {stage!r}, layout {layout!r}, order {order!r}, planes {planes!r}, dtype {dtype}")
        p, dt, mask = made
        if scale is None:
            sc = (1.0,) * 4
        elif np.ndim(scale) == 0:
            sc = (float(scale),) * 4
        else:
            sc = tuple(float(v) for v in scale)
            if len(sc) != 4:
                raise ValueError(f"frames_coef: scale {scale!r}: one number, or one each for Y, U, V, Y2")
        for c in range(4):
            p.scale[c] = np.float32(sc[c])
        size = int(self.L.vp8hip_coef_size(self.h, ctypes.byref(p)))
        if not size:
            raise ValueError(f"frames_coef: nfreq {nfreq} with layout {layout!r}, order {order!r}: refused (1..16; \"inplace\": 16, \"raster\")")
        flat = self._to_torch("frames_coef", [("out", out, _INT16_DTYPES[dt], (n, size // (2, 2, 4)[dt]))],
                              lambda arr_out, stride: self.L.vp8hip_frames_coef_async(
                                  self.h, (c_int * max(n, 1))(*slots), n, ctypes.byref(p), arr_out, stride),
                              "vp8hip_frames_coef_async")[0]
        return split_coef(flat, self.g.aligned_w // 16, self.g.aligned_h // 16, layout, mask, p.nfreq)

    def trace_pool(self, n):
        """a pool of n traces for frames_trace on the context's device: a torch.int16 tensor [n, d_h, d_w, 2], (x', y') per pixel of
        the display-size grid -- the position in the anchor picture the pixel descends from (include/vp8hip.h).  Not initialised."""
        torch, dev = self._torch_device("trace_pool")
        return torch.empty((int(n), self.height, self.width, 2), dtype=torch.int16, device=dev)

    def _trace_pool_args(self, who, pool, kind=("int16", 2)):
        """-> (dev, pointer, stride in bytes, entries) of a pool as trace_pool makes them (a view is fine: each entry dense); kind:
        the type's name and how many make a pixel's dword -- ("uint8", 4): a pool as wear_pool makes them; ("int32", 1): the COUNT
        pool of cover_pools, [n, d_h, d_w]"""
        torch, dev = self._torch_device(who)
        name, per = kind
        inner = (self.height, self.width) + ((per,) if per > 1 else ())
        if not (torch.is_tensor(pool) and pool.dim() == 1 + len(inner) and pool.shape[0] >= 1
                and self._dense(pool, getattr(torch, name), (pool.shape[0],) + inner, dev)):
            raise ValueError(f"{who}: pool must be {'an' if name[0] == 'i' else 'a'} {name} tensor [n, {', '.join(str(v) for v in inner)}], each entry dense, on {dev}")
        return dev, c_void_p(pool.data_ptr()), pool.stride(0) * (4 // per), int(pool.shape[0])

    def _chain_frames(self, who, jobs, pool, kind):
        """what frames_trace and frames_wear are: vp8hip_<who>_async over `jobs`, chaining the entries of a pool of `kind`
        (_trace_pool_args)"""
        arr, n = (jobs, len(jobs)) if isinstance(jobs, ctypes.Array) else (self.job_array(list(jobs)), len(jobs))
        dev, ptr, stride, entries = self._trace_pool_args(who, pool, kind)
        call = f"vp8hip_{who}_async"
        self._between_stream_waits(dev, lambda: getattr(self.L, call)(self.h, arr, n, ptr, stride, entries), call)
        return pool

    # what trace_flow, trace_wear and trace_cover differ in: the ctypes struct, the library's calls, the tensor types, the planes
    # there are (None: no choice, two always; then scale may be "pixels"), the scales and the pool's kind (_trace_pool_args)
    _ENTRY_CALLS = {"trace_flow": (TraceFlowParams, "vp8hip_trace_flow", _INT16_DTYPES, None, 2, ("int16", 2)),
                    "trace_wear": (TraceWearParams, "vp8hip_trace_wear", _RGB_DTYPES, WEAR_PLANES, 4, ("uint8", 4)),
                    "trace_cover": (TraceCoverParams, "vp8hip_trace_cover", _RGB_DTYPES, COVER_PLANES, 2, ("int32", 1))}

    def _trace_entries(self, who, pool, idx, width, height, planes, dtype, scale, out):
        """what trace_flow, trace_wear and trace_cover are: entries `idx` of `pool` as tensors [n, C, gh, gw] by the library's call"""
        import torch
        params, call, names, table, nscale, kind = self._ENTRY_CALLS[who]
        idx = [int(i) for i in idx]
        n = len(idx)
        dst_w, dst_h, gw, gh = self._trace_grid(who, width, height)
        dtype = getattr(torch, names[0]) if dtype is None else dtype
        dt, mask = _elem_dtype(dtype, names), 3 if table is None else _plane_mask(planes, table, False)
        if dt is None or mask is None:
            raise ValueError(f"{who}: dtype {dtype}" + ("" if table is None else f", planes {planes!r}"))
        if scale is None:
            sc = (1.0,) * nscale
        elif isinstance(scale, str):
            if table is not None or scale != "pixels":
                raise ValueError(f"{who}: scale {scale!r}")
            sc = (gw / self.width, gh / self.height)
        elif table is not None and np.ndim(scale) == 0:
            sc = (float(scale),) * nscale
        else:
            sc = tuple(float(v) for v in scale)
            if table is not None and len(sc) != nscale:
                raise ValueError(f"{who}: scale {scale!r}")
        p = params(dst_w, dst_h, dt) if table is None else params(dst_w, dst_h, dt, mask)
        for c in range(nscale):
            p.scale[c] = np.float32(sc[c])
        if not getattr(self.L, call + "_size")(self.h, ctypes.byref(p)):
            raise ValueError(f"{who}: grid {gw}x{gh}: refused (sizes 1..16383)")
        _, pptr, pstride, entries = self._trace_pool_args(who, pool, kind)
        return self._to_torch(who, [("out", out, names[dt], (n, bin(mask).count("1"), gh, gw))],
                              lambda arr_out, stride: getattr(self.L, call + "_async")(
                                  self.h, (c_int * max(n, 1))(*idx), n, ctypes.byref(p), pptr, pstride, entries, arr_out, stride),
                              call + "_async")[0]

    def frames_trace(self, jobs, pool):
        """The traces of `jobs` -- a list of (ir_slot, dst, (last, golden, alt)) as decode takes it, dst and the three references read
        as entries of `pool` (trace_pool; -1 or refs None: no trace) -- written into pool[dst] (vp8hip_frames_trace_async): a key
        frame's is the identity, an inter frame's follows each pixel's vector, rounded to whole pixels and clamped to the picture,
        into the trace of the reference its macroblock was predicted from.  A pool numbered like the frame buffers takes the very
        jobs of decode (a vp8hip_job array made by job_array is taken as it is).  Jobs of one call are independent.  Stream
        ordering, the `import torch` first rule and the remark on record_stream: as frames_scaled.  Returns pool."""
        return self._chain_frames("frames_trace", jobs, pool, ("int16", 2))

    def trace_flow(self, pool, idx, width=None, height=None, dtype=None, scale=None, out=None):
        """Entries `idx` of `pool` (any order, repeats allowed) as flow tensors [n, 2, gh, gw] on the context's device
        (vp8hip_trace_flow_async): channel 0 = x' - x, channel 1 = y' - y in whole display pixels, signed as frames_side's vectors,
        at the display size or under each output's centre at width x height (then the tensor lines up with frames_rgb's and
        frames_side's at that size).  torch.int16 (the default), torch.float16 or torch.float32; float types:
        float32(float64(a) * scale[c]) with scale = (x, y) float32 numbers (default 1, 1); scale="pixels" is (gw / d_w, gh / d_h),
        computed in float64 and rounded once: the flow in pixels of the tensor.  `out`: a tensor of that shape and type, each
        frame dense, stride(0) free.  Stream ordering: as frames_scaled."""
        return self._trace_entries("trace_flow", pool, idx, width, height, None, dtype, scale, out)

    def wear_pool(self, n):
        """a pool of n wear entries for frames_wear on the context's device: a torch.uint8 tensor [n, d_h, d_w, 4], the counters (hops,
        intra, edge, coded) per pixel of the display-size grid (include/vp8hip.h).  Not initialised."""
        torch, dev = self._torch_device("wear_pool")
        return torch.empty((int(n), self.height, self.width, 4), dtype=torch.uint8, device=dev)

    def frames_wear(self, jobs, pool):
        """The wear of `jobs` -- the jobs of frames_trace, dst and the three references read as entries of `pool` (wear_pool; -1 or
        refs None: no entry) -- written into pool[dst] (vp8hip_frames_wear_async): what happened to each pixel on the way its trace
        takes to the anchor picture, four saturating byte counters -- every hop; the hops in which its macroblock was intra (held
        in place); those in which the clamp moved the position; those in which its luma block may have had a residual.  A key
        frame's is zero; an inter frame's is the wear of the reference at the position the trace's hop goes to, plus the hop's
        increments.  A pool numbered like the trace pool takes the very jobs of frames_trace.  Stream ordering: as frames_trace.
        Returns pool."""
        return self._chain_frames("frames_wear", jobs, pool, ("uint8", 4))

    def trace_wear(self, pool, idx, width=None, height=None, planes=("hops", "intra", "edge", "coded"), dtype=None, scale=None, out=None):
        """Entries `idx` of the wear pool `pool` (any order, repeats allowed) as tensors [n, C, gh, gw] on the context's device
        (vp8hip_trace_wear_async): the counters of `planes` ("hops", "intra", "edge", "coded", or the mask) in bit order, at the
        display size or under each output's centre at width x height (then the tensor lines up with trace_flow's, trace_gather's
        and frames_rgb's at that size).  torch.uint8 (the default: the counter), torch.float16 or torch.float32; float types:
        float32(float64(v) * scale[c]) with scale = one number or four, by counter (hops, intra, edge, coded) whatever planes are
        asked for, float32 (default 1).  `out`: a tensor of that shape and type, each frame dense, stride(0) free.  Stream
        ordering: as frames_scaled."""
        return self._trace_entries("trace_wear", pool, idx, width, height, planes, dtype, scale, out)

    def cover_pools(self, n):
        """(FIRST, COUNT): pools of n entries each for trace_invert on the context's device.  FIRST is a torch.int16 tensor
        [n, d_h, d_w, 2], exactly what trace_pool returns: (x, y) of the first frame pixel that descends from the anchor pixel,
        (-1, -1) where none does.  COUNT is a torch.int32 tensor [n, d_h, d_w]: how many do.  Not initialised."""
        torch, dev = self._torch_device("cover_pools")
        return self.trace_pool(n), torch.empty((int(n), self.height, self.width), dtype=torch.int32, device=dev)

    def trace_invert(self, pool, jobs, first=None, count=None):
        """The traces of `pool` inverted (vp8hip_trace_invert_async).  `jobs`: a list of (entry, dst): the entry of `pool` that holds a
        frame's trace (frames_trace) and the entry of `first` and of `count` (cover_pools; either may be None, not both) its
        inverse is written into; repeats of an entry are allowed, every dst once.  For every pixel of the ANCHOR's grid, first[dst]
        holds the first pixel of the frame in raster order whose trace, clamped to the picture, names it -- packed as a trace, so
        trace_flow and trace_gather read `first` as a pool of traces in the other direction; (-1, -1) where there is none -- and
        count[dst] how many there are.  The pools must not overlap.  Stream ordering: as frames_trace.  Returns (first, count)
        as passed."""
        arr, n = self._trace_jobs("trace_invert", jobs, InvertJob, "(entry, dst)")
        if first is None and count is None:
            raise ValueError("trace_invert: first, count or both")
        dev, pptr, pstride, entries = self._trace_pool_args("trace_invert", pool)
        fptr, fstride, fn = None, 0, None
        cptr, cstride, cn = None, 0, None
        if first is not None:
            _, fptr, fstride, fn = self._trace_pool_args("trace_invert (first)", first)
        if count is not None:
            _, cptr, cstride, cn = self._trace_pool_args("trace_invert (count)", count, ("int32", 1))
        if fn is not None and cn is not None and fn != cn:
            raise ValueError(f"trace_invert: first has {fn} entries, count {cn}")
        out_frames = fn if fn is not None else cn
        self._between_stream_waits(dev, lambda: self.L.vp8hip_trace_invert_async(self.h, arr, n, pptr, pstride, entries, fptr, fstride, cptr,
                                                                                 cstride, out_frames), "vp8hip_trace_invert_async")
        return first, count

    def trace_cover(self, count, idx, width=None, height=None, planes=("count", "seen"), dtype=None, scale=None, out=None):
        """Entries `idx` of the COUNT pool `count` (trace_invert; any order, repeats allowed) as tensors [n, C, gh, gw] on the
        context's device (vp8hip_trace_cover_async): the planes of `planes` ("count": min(count, 255); "seen": count != 0; or the
        mask) in bit order, at the display size or under each output's centre at width x height (then the tensor lines up with
        trace_flow's and trace_gather's of a FIRST pool at that size).  torch.uint8 (the default), torch.float16 or torch.float32;
        float types: float32(float64(v) * scale[c]) with scale = one number or two, by plane (count, seen) whatever planes are
        asked for, float32 (default 1).  `out`: a tensor of that shape and type, each frame dense, stride(0) free.  Stream
        ordering: as frames_scaled."""
        return self._trace_entries("trace_cover", count, idx, width, height, planes, dtype, scale, out)

    @staticmethod
    def _hist_args(who, items, planes, table):
        """-> (how many jobs, the plane mask, how many planes) of a histogram call; ValueError for no job, no plane or an unknown one"""
        mask = _plane_mask(planes, table, False)
        if mask is None:
            raise ValueError(f"{who}: planes {planes!r} (at least one of {', '.join(table)})")
        if len(items) < 1:
            raise ValueError(f"{who}: no jobs")
        return len(items), mask, bin(mask).count("1")

    def _hist(self, who, call, n, nplanes, out, fn):
        """what the four histogram calls end in: the torch.int32 tensor [n, planes, 256] -- `out` when given, each job's counts
        dense, stride(0) free -- filled by fn(pointer, stride in bytes) between the stream waits"""
        return self._to_torch(who, [("out", out, "int32", (n, nplanes, 256))], fn, call)[0]

    @staticmethod
    def _pair_jobs(who, jobs, planes, table, none_ok=False, ref_optional=False):
        """-> (the HistJob array, how many jobs, the plane mask) of a call over picture pairs (frames_hist, frames_ssim, frames_motion, frames_subpel,
        frames_tfilter, frames_quant);
        ValueError, in this order, for a job that is no (fb, ref_fb) -- ref_optional: or a bare frame buffer, and ref_fb may be
        None --, for an unknown plane or -- unless none_ok -- no plane, for no job and for a negative frame buffer"""
        items = []
        for j in jobs:
            if ref_optional:
                j = (j, None) if isinstance(j, (int, np.integer)) else tuple(j)
            if not isinstance(j, (tuple, list)) or len(j) != 2:
                raise ValueError(f"{who}: jobs are {'frame buffers or ' if ref_optional else ''}(fb, ref_fb)")
            items.append((int(j[0]), -1 if ref_optional and j[1] is None else int(j[1])))
        mask = _plane_mask(planes, table, none_ok)
        if mask is None:
            raise ValueError(f"{who}: planes {planes!r} ({'of' if none_ok else 'at least one of'} {', '.join(table)})")
        if not items:
            raise ValueError(f"{who}: no jobs")
        if any(fb < 0 or ref < (-1 if ref_optional else 0) for fb, ref in items):
            raise ValueError(f"{who}: a negative frame buffer{' (ref_fb: None or -1 for none)' if ref_optional else ''}")
        return (HistJob * len(items))(*items), len(items), mask

    def frames_hist(self, jobs, planes=("y", "u", "v"), out=None):
        """Byte histograms of pictures on the context's device (vp8hip_frames_hist_async): a torch.int32 tensor [n, P, 256].  `jobs`:
        a list of frame buffers, or of (fb, ref_fb) with ref_fb None or -1 for none (any order, repeats allowed).  Without a
        reference H[i, p, k] counts the samples of plane p of frame buffer fb -- as frames_scaled hands it out at the display size --
        that equal k; with one, the sample positions where |fb - ref_fb| equals k, from which SAD, SSE and PSNR follow exactly.
        planes: "y", "u", "v" (or the mask), in that order.  Each frame buffer is read in the form it has; nothing is converted or
        allocated.  Counts are below 2^28.  Stream ordering, the `import torch` first rule and the remark on record_stream: as
        frames_scaled."""
        who = "frames_hist"
        arr, n, mask = self._pair_jobs(who, jobs, planes, HIST_PLANES, ref_optional=True)
        return self._hist(who, "vp8hip_frames_hist_async", n, bin(mask).count("1"), out,
                          lambda ptr, stride: self.L.vp8hip_frames_hist_async(self.h, arr, n, mask, ptr, stride))

    def slots_hist(self, slots, planes, out=None):
        """Byte histograms of IR slots' info planes on the context's device (vp8hip_slots_hist_async): a torch.int32 tensor [n, P, 256],
        H[i, p, k] the number of cells of the native grid (a cell per 4x4 luma block of the coded area) whose value in plane p of
        frames_side's info tensor equals k.  planes: frames_side's ("ref", "mode", "skip", "segment", "qindex", "coded") and "mvmag",
        the larger component of the cell's vector in whole pixels, rounded as the trace rounds and capped at 255 (0 on key frames
        and intra macroblocks); or the mask; always in bit order, "mvmag" last.  Stream ordering: as frames_scaled."""
        who = "slots_hist"
        slots = [int(s) for s in slots]
        n, mask, nplanes = self._hist_args(who, slots, planes, SLOT_HIST_PLANES)
        if any(s < 0 for s in slots):
            raise ValueError(f"{who}: a negative slot")
        arr = (c_int * n)(*slots)
        return self._hist(who, "vp8hip_slots_hist_async", n, nplanes, out,
                          lambda ptr, stride: self.L.vp8hip_slots_hist_async(self.h, arr, n, mask, ptr, stride))

    def _entries_hist(self, who, pool, idx, planes, out):
        """what trace_wear_hist and trace_cover_hist are: the histograms of entries `idx` of `pool` by the library's call"""
        _, call, _, table, _, kind = self._ENTRY_CALLS[who[:-5]]
        idx = [int(i) for i in idx]
        n, mask, nplanes = self._hist_args(who, idx, planes, table)
        if any(i < 0 for i in idx):
            raise ValueError(f"{who}: a negative entry")
        _, pptr, pstride, entries = self._trace_pool_args(who, pool, kind)
        if any(i >= entries for i in idx):
            raise ValueError(f"{who}: an entry outside the pool's {entries}")
        arr = (c_int * n)(*idx)
        return self._hist(who, call + "_hist_async", n, nplanes, out,
                          lambda ptr, stride: getattr(self.L, call + "_hist_async")(self.h, arr, n, mask, pptr, pstride, entries, ptr, stride))

    def trace_wear_hist(self, pool, idx, planes=("hops", "intra", "edge", "coded"), out=None):
        """Byte histograms of wear entries on the context's device (vp8hip_trace_wear_hist_async): a torch.int32 tensor [n, P, 256],
        H[i, p, k] the number of pixels of entry idx[i] of the wear pool `pool` whose counter p -- trace_wear's planes, in bit order
        -- equals k.  What a scheduler reads to decide when to re-anchor, without trace_wear's tensor.  `out` must not overlap the
        pool.  Stream ordering: as frames_scaled."""
        return self._entries_hist("trace_wear_hist", pool, idx, planes, out)

    def trace_cover_hist(self, count, idx, planes=("count", "seen"), out=None):
        """Byte histograms of COUNT entries on the context's device (vp8hip_trace_cover_hist_async): a torch.int32 tensor [n, P, 256]
        over trace_cover's planes at the display size: "count" is min(count, 255), "seen" fills bins 0 and 1 only -- H[i, p, 1] of
        "seen" is how many anchor pixels survive into the frame.  `out` must not overlap the pool.  Stream ordering: as
        frames_scaled."""
        return self._entries_hist("trace_cover_hist", count, idx, planes, out)

    def frames_ssim(self, jobs, planes=("y", "u", "v"), map_dtype=None, out_scores=None, out_map=None):
        """The structural similarity of picture pairs on the context's device (vp8hip_frames_ssim_async): vp8_ssim2's 8x8 windows on
        the 4-pixel grid over the display-size planes, in the reference's integer definition.  `jobs`: a list of (fb, ref_fb), any
        order, repeats allowed, fb == ref_fb legal.  planes: "y", "u", "v" (or the mask), in that order.  Returns the scores, a
        torch.int64 tensor [n, P, 2]: [i, p, 0] the sum over plane p's windows of the window value in Q32 (rounded half to even),
        [i, p, 1] the number of windows -- ssim_mean gives the means, ssim_combined the reference's two weightings --; the same bits
        in every run.  With map_dtype (torch.float16 / torch.float32, or SSIM_F16 / SSIM_F32) returns (scores, map): the window
        values themselves, a tensor [n, elems] of that type, the planes back to back, each a dense [nwy, nwx] (split_ssim_map gives
        the views; ssim_windows the sizes).  Each frame buffer is read in the form it has; nothing is converted or allocated.
        `out_scores`, `out_map`: tensors of those shapes and types, each job dense, stride(0) free.  Stream ordering, the `import
        torch` first rule and the remark on record_stream: as frames_scaled."""
        who = "frames_ssim"
        arr, n, mask = self._pair_jobs(who, jobs, planes, HIST_PLANES)
        nplanes = bin(mask).count("1")
        dt = 0 if map_dtype is None else _ssim_dtype(map_dtype)
        if dt is None or (out_map is not None and not dt):
            raise ValueError(f"{who}: map_dtype {map_dtype!r} (float16 or float32; out_map needs one)")
        p = SsimParams(mask, dt)
        outs = [("out_scores", out_scores, "int64", (n, nplanes, 2))]
        if dt:
            size = int(self.L.vp8hip_ssim_map_size(self.h, ctypes.byref(p)))
            if not size:
                raise ValueError(f"{who}: planes {planes!r} of {self.width}x{self.height} have no windows: no map")
            outs.append(("out_map", out_map, _SSIM_DTYPES[dt], (n, size // (0, 2, 4)[dt])))
        made = self._to_torch(who, outs, lambda sp, ss, mp=None, ms=0: self.L.vp8hip_frames_ssim_async(self.h, arr, n, ctypes.byref(p), sp, ss, mp, ms),
                              "vp8hip_frames_ssim_async")
        return tuple(made) if dt else made[0]

    def frames_motion(self, jobs, distance=16, centre=None, cost=None, sad_per_bit=0, planes=("sad",), out_mv=None, out_stats=None):
        """Full-search block motion between picture pairs on the context's device (vp8hip_frames_motion_async): per macroblock of fb
        the whole-pixel vector into ref_fb that the reference's vp8_full_search_sad_c finds within `distance` (1..64) of the centre,
        bit for bit.  `jobs`: a list of (fb, ref_fb), any order, repeats allowed, fb == ref_fb legal.  Returns (mv, stats): mv a
        torch.int16 tensor [n, 2, mb_rows, mb_cols], channel 0 = x, 1 = y, in 1/8 pel like frames_side's vectors; stats a
        torch.int32 tensor [n, P, mb_rows, mb_cols] holding uint32 bits, the planes of `planes` ("sad": the best value; "sad0": the
        SAD at (0, 0); "sse" and "var" at the best vector; "srcvar": the block's activity; or the mask) in bit order -- None
        where planes is empty.  `centre`: a torch.int16 tensor [n, 2, mb_rows, mb_cols] of search centres in whole pixels (x, y) on
        the device, each job dense; None: (0, 0).  `cost`: int32 [2, 2 * distance + 1], row costs then column costs (0..65535), with
        sad_per_bit (0..255) the reference's mvsad_err_cost around the centre; None or sad_per_bit 0: plain SAD.  Each frame buffer
        is read in the form it has; nothing is converted or allocated.  `out_mv`, `out_stats`: tensors of those shapes and types,
        each job dense, stride(0) free.  Stream ordering, the `import torch` first rule and the remark on record_stream: as
        frames_scaled."""
        who = "frames_motion"
        arr, n, mask = self._pair_jobs(who, jobs, planes, MOTION_PLANES, none_ok=True)
        d, spb = int(distance), int(sad_per_bit)
        if not 1 <= d <= MOTION_MAX_DISTANCE or not 0 <= spb <= 255:
            raise ValueError(f"{who}: distance {distance} (1..{MOTION_MAX_DISTANCE}), sad_per_bit {sad_per_bit} (0..255)")
        if out_stats is not None and not mask:
            raise ValueError(f"{who}: out_stats without planes")
        table = None
        if cost is not None:
            table = np.ascontiguousarray(cost, dtype=np.int32)
            if table.shape != (2, 2 * d + 1) or (table < 0).any() or (table > 65535).any():
                raise ValueError(f"{who}: cost is int32 [2, {2 * d + 1}] of 0..65535")
        rows, cols = self.g.aligned_h // 16, self.g.aligned_w // 16
        p = MotionParams(d, spb, mask, None if table is None else table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        cptr, cstride = None, 0
        if centre is not None:
            torch, dev = self._torch_device(who)
            if not self._dense(centre, torch.int16, (n, 2, rows, cols), dev):
                raise ValueError(f"{who}: centre must be an int16 tensor {[n, 2, rows, cols]}, each job dense, on {dev}")
            cptr, cstride = c_void_p(centre.data_ptr()), centre.stride(0) * 2
        outs = [("out_mv", out_mv, "int16", (n, 2, rows, cols))]
        if mask:
            outs.append(("out_stats", out_stats, "int32", (n, bin(mask).count("1"), rows, cols)))
        made = self._to_torch(who, outs, lambda vp, vs, sp=None, ss=0: self.L.vp8hip_frames_motion_async(self.h, arr, n, ctypes.byref(p), cptr, cstride,
                                                                                                         vp, vs, sp, ss),
                              "vp8hip_frames_motion_async")
        return made[0], (made[1] if mask else None)

    def frames_subpel(self, jobs, start=None, ref=None, cost=None, error_per_bit=0, precision=4, planes=("val",), out_mv=None, out_stats=None):
        """Sub-pixel refinement of block motion between picture pairs on the context's device (vp8hip_frames_subpel_async): per
        macroblock of fb the vector into ref_fb that the reference's vp8_find_best_sub_pixel_step (precision 4: half, then quarter
        pel; precision 2: vp8_find_best_half_pixel_step) finds around a whole-pixel start, bit for bit.  `jobs`: a list of
        (fb, ref_fb), any order, repeats allowed, fb == ref_fb legal.  Returns (mv, stats): mv a torch.int16 tensor
        [n, 2, mb_rows, mb_cols], channel 0 = x, 1 = y, in 1/8 pel like frames_side's and frames_motion's vectors; stats a
        torch.int32 tensor [n, P, mb_rows, mb_cols] holding uint32 bits, the planes of `planes` ("val": the best value, cost
        included; "var" and "sse" at the best vector; "var0": the variance at the start; or the mask) in bit order -- None where
        planes is empty.  `start`: a torch.int16 tensor [n, 2, mb_rows, mb_cols] in 1/8 pel on the device, each job dense --
        frames_motion's mv as it stands: frames_subpel(jobs, start=frames_motion(jobs)[0]) is the reference's two steps --; None:
        (0, 0).  `cost`: int32 [2, 2 R + 1], row costs then column costs (0..65535), R = 1..1023, with error_per_bit (0..16383) the
        reference's mv_err_cost counted from `ref`, a tensor of start's shape and units (None: (0, 0)); cost None or error_per_bit
        0: the plain variance.  Each frame buffer is read in the form it has; nothing is converted, and only a call with a cost
        table adds device memory: 8 KB, once per context.  `out_mv`, `out_stats`: tensors of those shapes and types, each job
        dense, stride(0) free.  Stream ordering, the `import torch` first rule and the remark on record_stream: as frames_scaled."""
        who = "frames_subpel"
        arr, n, mask = self._pair_jobs(who, jobs, planes, SUBPEL_PLANES, none_ok=True)
        epb, prec = int(error_per_bit), int(precision)
        if prec not in (2, 4) or not 0 <= epb <= SUBPEL_MAX_ERROR_PER_BIT:
            raise ValueError(f"{who}: precision {precision} (2 or 4), error_per_bit {error_per_bit} (0..{SUBPEL_MAX_ERROR_PER_BIT})")
        if out_stats is not None and not mask:
            raise ValueError(f"{who}: out_stats without planes")
        table, rng = None, 0
        if cost is not None:
            table = np.ascontiguousarray(cost, dtype=np.int32)
            rng = (table.shape[1] - 1) // 2 if table.ndim == 2 else 0
            if table.ndim != 2 or table.shape != (2, 2 * rng + 1) or not 1 <= rng <= SUBPEL_MAX_COST_RANGE or (table < 0).any() or (table > 65535).any():
                raise ValueError(f"{who}: cost is int32 [2, 2 R + 1] of 0..65535, R = 1..{SUBPEL_MAX_COST_RANGE}")
        rows, cols = self.g.aligned_h // 16, self.g.aligned_w // 16
        p = SubpelParams(prec, epb, rng, mask, None if table is None else table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        ins = []
        for name, t in (("start", start), ("ref", ref)):
            if t is None:
                ins += [None, 0]
                continue
            torch, dev = self._torch_device(who)
            if not self._dense(t, torch.int16, (n, 2, rows, cols), dev):
                raise ValueError(f"{who}: {name} must be an int16 tensor {[n, 2, rows, cols]}, each job dense, on {dev}")
            ins += [c_void_p(t.data_ptr()), t.stride(0) * 2]
        outs = [("out_mv", out_mv, "int16", (n, 2, rows, cols))]
        if mask:
            outs.append(("out_stats", out_stats, "int32", (n, bin(mask).count("1"), rows, cols)))
        made = self._to_torch(who, outs, lambda vp, vs, sp=None, ss=0: self.L.vp8hip_frames_subpel_async(self.h, arr, n, ctypes.byref(p), *ins, vp, vs,
                                                                                                         sp, ss),
                              "vp8hip_frames_subpel_async")
        return made[0], (made[1] if mask else None)

    def frames_tfilter(self, jobs, pairs, mv=None, err=None, strength=3, filter="sixtap", thresh=(10000, 20000), want_count=False, out=None,
                       out_count=None):
        """The reference's motion-compensated temporal filter (ARNR) of pictures on the context's device
        (vp8hip_frames_tfilter_async): each centre picture blended with the motion-compensated predictions from its sources, pixel by
        pixel, a prediction trusted less the further it lies from the centre's pixel, bit for bit with
        vp8/encoder/temporal_filter.c.  `pairs`: the list of (fb, ref_fb) given to frames_motion / frames_subpel, ref_fb the source.
        `jobs`: a list of (fb, first, count): the centre fb over pairs first .. first + count - 1 (count 1..15), all of them pairs
        of fb; jobs may share pairs; the centre takes part where (fb, fb) is listed.  `mv`: frames_subpel's (or frames_motion's)
        torch.int16 tensor [npairs, 2, mb_rows, mb_cols] as it stands, None: (0, 0).  `err`: a torch.int32 tensor
        [npairs, mb_rows, mb_cols] holding uint32 bits, or the [npairs, 1, mb_rows, mb_cols] stats of frames_subpel(planes=("val",))
        as it stands; a source weighs 2 below thresh[0], 1 below thresh[1], else 0, per macroblock; None: 2.  strength: 0..6;
        filter: "sixtap" or "bilinear".  Returns a torch.uint8 tensor [n, i420_size(width, height)] -- frames_scaled's layout at the
        display size: split_i420 gives the planes -- and with want_count (or out_count) also the per-pixel count, a torch.int16
        tensor of the same shape holding uint16 bits (32 per fully trusted source).  Each frame buffer is read in the form it has;
        nothing is converted or allocated.  `out` as for frames_scaled (stride(1) == 1), `out_count` likewise.  Stream ordering, the
        `import torch` first rule and the remark on record_stream: as frames_scaled."""
        who = "frames_tfilter"
        pairs = list(pairs)
        parr, npairs, _ = self._pair_jobs(who, pairs, 0, {}, none_ok=True)
        centres = [int(pair[0]) for pair in pairs]
        items = []
        for j in jobs:
            if not isinstance(j, (tuple, list)) or len(j) != 3:
                raise ValueError(f"{who}: jobs are (fb, first, count)")
            items.append(tuple(int(v) for v in j))
        if not items:
            raise ValueError(f"{who}: no jobs")
        for fb, first, count in items:
            if fb < 0 or not 1 <= count <= TFILTER_MAX_COUNT or first < 0 or first + count > npairs:
                raise ValueError(f"{who}: job {(fb, first, count)}: count 1..{TFILTER_MAX_COUNT}, pairs inside the list's {npairs}")
            if any(c != fb for c in centres[first:first + count]):
                raise ValueError(f"{who}: job {(fb, first, count)} takes a pair of another frame buffer")
        n = len(items)
        if isinstance(filter, str) and filter not in TFILTER_FILTERS:
            raise ValueError(f"{who}: filter {filter!r} ({', '.join(TFILTER_FILTERS)})")
        flt = TFILTER_FILTERS[filter] if isinstance(filter, str) else int(filter)
        lo, hi = (int(t) for t in thresh)
        if not 0 <= int(strength) <= 6 or flt not in (0, 1) or not 0 <= lo <= hi < 1 << 32:
            raise ValueError(f"{who}: strength {strength} (0..6), filter {filter!r}, thresh {thresh!r} (0 <= low <= high < 2^32)")
        p = TfilterParams(int(strength), flt, lo, hi)
        rows, cols = self.g.aligned_h // 16, self.g.aligned_w // 16
        ins = []
        for name, t, kind, shapes in (("mv", mv, "int16", [(npairs, 2, rows, cols)]),
                                      ("err", err, "int32", [(npairs, rows, cols), (npairs, 1, rows, cols)])):
            if t is None:
                ins += [None, 0]
                continue
            torch, dev = self._torch_device(who)
            if not any(self._dense(t, getattr(torch, kind), shape, dev) for shape in shapes):
                raise ValueError(f"{who}: {name} must be an {kind} tensor {' or '.join(str(list(sh)) for sh in shapes)}, each pair dense, on {dev}")
            ins += [c_void_p(t.data_ptr()), t.stride(0) * t.element_size()]
        size = int(self.L.vp8hip_i420_size(self.width, self.height))
        counted = bool(want_count) or out_count is not None

        def ok(out, dtype, shape, dev):
            return out.dtype == dtype and out.dim() == 2 and tuple(out.shape) == tuple(shape) and out.stride(1) == 1 and out.device == dev
        outs = [("out", out, "uint8", (n, size))]
        if counted:
            outs.append(("out_count", out_count, "int16", (n, size)))
        jarr = (TfilterJob * n)(*items)
        made = self._to_torch(who, outs, lambda dp, ds, cp=None, cs=0: self.L.vp8hip_frames_tfilter_async(self.h, jarr, n, parr, npairs, ctypes.byref(p),
                                                                                                         *ins, dp, ds, cp, cs),
                              "vp8hip_frames_tfilter_async", ok, "with stride(1) == 1")
        return tuple(made) if counted else made[0]

    def frames_quant(self, jobs, mv=None, qindex=40, deltas=(0, 0, 0, 0, 0), quantizer="regular", filter="sixtap", stage="levels",
                     zbin=(0, 0, 0), planes=(), want=("coef", "eob"), out_coef=None, out_eob=None, out_stats=None, out_rec=None):
        """The reference's inter 16x16 encode of picture pairs on the context's device (vp8hip_frames_quant_async): per macroblock
        of fb the prediction from ref_fb at the vector, the residual, the forward DCT and Walsh transform, the quantiser and --
        where asked -- the reconstruction, bit for bit with vp8_encode_inter16x16, vp8_inverse_transform_mby and
        vp8_dequant_idct_add_uv_block.  `jobs`: a list of (fb, ref_fb), fb the source, ref_fb the reference; any order, repeats
        allowed, fb == ref_fb legal.  `mv`: frames_subpel's (or frames_motion's) torch.int16 tensor [n, 2, mb_rows, mb_cols] as it
        stands, None: (0, 0).  `qindex`: 0..127 for every job, or a sequence of n, one a job.  `deltas`: y1dc, y2dc, y2ac, uvdc,
        uvac, each -15..15 (the reference's rule that y2dc is 4 - Q below Q 4 is the caller's to apply).  quantizer: "regular" or
        "fast"; filter: "sixtap" or "bilinear"; stage: "levels" or "dequant", what coef holds; zbin: (zbin_over_quant,
        zbin_mode_boost, act_zbin_adj), the regular quantiser's.  Returns a dict of what `want` names or an out_* tensor is given
        for: "coef" a torch.int16 tensor [n, mb_rows, mb_cols, 25, 16] (blocks Y 0..15, U 16..19, V 20..23, Y2 24; position
        4 v + u), "eob" torch.uint8 [n, mb_rows, mb_cols, 32] (entries 25..31 are 0), "stats" torch.int32
        [n, P, mb_rows, mb_cols] holding uint32 bits, the planes of `planes` ("erry", "erry2", "erruv", "eobs", "recsse", or the
        mask) in bit order -- asked for by naming planes --, "rec" torch.uint8 [n, i420_size(width, height)], frames_tfilter's
        layout.  Without "rec" and "recsse" no inverse transform is made.  Each frame buffer is read in the form it has; nothing
        is converted or allocated.  out_*: tensors of those shapes and types, each job dense, stride(0) free (a multiple of 16
        bytes for coef, 4 for eob).  Stream ordering, the `import torch` first rule and the remark on record_stream: as
        frames_scaled."""
        who = "frames_quant"
        arr, n, mask = self._pair_jobs(who, jobs, planes, QUANT_PLANES, none_ok=True)
        want = {want} if isinstance(want, str) else set(want)
        if want - {"coef", "eob", "stats", "rec"}:
            raise ValueError(f"{who}: want {sorted(want)!r} (of coef, eob, stats, rec)")
        given = {"coef": out_coef, "eob": out_eob, "stats": out_stats, "rec": out_rec}
        want |= {k for k, t in given.items() if t is not None}
        if mask:
            want.add("stats")
        if "stats" in want and not mask:
            raise ValueError(f"{who}: stats without planes")
        if not want:
            raise ValueError(f"{who}: no output asked for")
        jq = None
        if isinstance(qindex, (int, np.integer)):
            qs = [int(qindex)]
        else:
            qs = [int(q) for q in qindex]
            if len(qs) != n:
                raise ValueError(f"{who}: {len(qs)} qindex values for {n} jobs")
            jq = (ctypes.c_uint8 * n)(*[q & 255 for q in qs])
        d = [int(v) for v in deltas]
        z = [int(v) for v in zbin]
        if any(not 0 <= q <= 127 for q in qs) or len(d) != 5 or any(not -15 <= v <= 15 for v in d):
            raise ValueError(f"{who}: qindex {qindex!r} (0..127), deltas {deltas!r} (five of -15..15)")
        if len(z) != 3 or any(abs(v) > QUANT_ZBIN_MAX for v in z):
            raise ValueError(f"{who}: zbin {zbin!r} (zbin_over_quant, zbin_mode_boost, act_zbin_adj, each within +-{QUANT_ZBIN_MAX})")
        if quantizer not in QUANT_QUANTIZERS or filter not in TFILTER_FILTERS or stage not in COEF_STAGES:
            raise ValueError(f"{who}: quantizer {quantizer!r} ({', '.join(QUANT_QUANTIZERS)}), filter {filter!r} ({', '.join(TFILTER_FILTERS)}), "
                             f"stage {stage!r} ({', '.join(COEF_STAGES)})")
        p = QuantParams(qs[0], (c_int * 5)(*d), QUANT_QUANTIZERS[quantizer], TFILTER_FILTERS[filter], COEF_STAGES[stage], z[0], z[1], z[2], mask or 0, jq)
        rows, cols = self.g.aligned_h // 16, self.g.aligned_w // 16
        mptr, mstride = None, 0
        if mv is not None:
            torch, dev = self._torch_device(who)
            if not self._dense(mv, torch.int16, (n, 2, rows, cols), dev):
                raise ValueError(f"{who}: mv must be an int16 tensor {[n, 2, rows, cols]}, each job dense, on {dev}")
            mptr, mstride = c_void_p(mv.data_ptr()), mv.stride(0) * 2
        shapes = {"coef": ("int16", (n, rows, cols, 25, 16)), "eob": ("uint8", (n, rows, cols, 32)),
                  "stats": ("int32", (n, bin(mask or 0).count("1"), rows, cols)),
                  "rec": ("uint8", (n, int(self.L.vp8hip_i420_size(self.width, self.height))))}
        names = [k for k in ("coef", "eob", "stats", "rec") if k in want]
        outs = [("out_" + k, given[k], shapes[k][0], shapes[k][1]) for k in names]

        def call(*args):
            a = dict(zip(names, zip(args[0::2], args[1::2])))
            flat = [v for k in ("coef", "eob", "stats", "rec") for v in a.get(k, (None, 0))]
            return self.L.vp8hip_frames_quant_async(self.h, arr, n, ctypes.byref(p), mptr, mstride, *flat)
        made = self._to_torch(who, outs, call, "vp8hip_frames_quant_async")
        return dict(zip(names, made))

    def frames_intra(self, fbs, qindex=40, deltas=(0, 0, 0, 0, 0), quantizer="regular", stage="levels", zbin=(0, 0, 0), rdmult=None, rddiv=None,
                     mbmode_cost=None, bmode_cost=None, bmode_last=3, bpred=True, planes=(), want=("coef", "eob", "modes"), out_coef=None,
                     out_eob=None, out_stats=None, out_rec=None, out_modes=None):
        """The reference's intra mode decision and encode of key-frame macroblocks on the context's device
        (vp8hip_frames_intra_async): per macroblock of each source picture vp8_pick_intra_mode -- the chroma mode, the 16x16 mode,
        the B_PRED chain, the choice -- then the encode and the unfiltered reconstruction the neighbours predict from, bit for bit.
        `fbs`: a list of frame buffers, the sources; any order, repeats allowed.  qindex, deltas, quantizer, stage, zbin: as
        frames_quant.  rdmult (0..1000), rddiv (1..100): None for intra_rd(qindex, deltas[0], zbin[0]) -- one pair serves every job
        of a call, so with a sequence of DIFFERENT qindex values both must be given --; mbmode_cost [5], bmode_cost [10, 10, 10], each 0..65535: None for intra_costs().  bmode_last:
        the last sub-block mode tried, 0..9; the reference's is 3.  bpred=False leaves the B_PRED chain out.  Returns a dict of what
        `want` names or an out_* tensor is given for: "coef", "eob", "rec" as frames_quant (a B_PRED macroblock codes position 0 of
        its luma blocks and has a zero block 24), "modes" torch.uint8 [n, mb_rows, mb_cols, 32] ([0] y mode, [1] uv mode, [2]
        skippable, [4..19] the sub-block modes), "stats" torch.int32 [n, P, mb_rows, mb_cols] holding uint32 bits, the planes of
        `planes` ("rd16", "rd4", "rate", "eobs", "recsse", or the mask) in bit order.  out_*: as frames_quant (modes: stride(0) a
        multiple of 4).  Stream ordering, the `import torch` first rule and the remark on record_stream: as frames_scaled."""
        who = "frames_intra"
        fbs = [int(f) for f in fbs]
        n = len(fbs)
        mask = _plane_mask(planes, INTRA_PLANES, True)
        if mask is None:
            raise ValueError(f"{who}: planes {planes!r} (of {', '.join(INTRA_PLANES)})")
        if not n:
            raise ValueError(f"{who}: no jobs")
        if any(f < 0 for f in fbs):
            raise ValueError(f"{who}: a negative frame buffer")
        want = {want} if isinstance(want, str) else set(want)
        if want - {"coef", "eob", "stats", "rec", "modes"}:
            raise ValueError(f"{who}: want {sorted(want)!r} (of coef, eob, stats, rec, modes)")
        given = {"coef": out_coef, "eob": out_eob, "stats": out_stats, "rec": out_rec, "modes": out_modes}
        want |= {k for k, t in given.items() if t is not None}
        if mask:
            want.add("stats")
        if "stats" in want and not mask:
            raise ValueError(f"{who}: stats without planes")
        if not want:
            raise ValueError(f"{who}: no output asked for")
        jq = None
        if isinstance(qindex, (int, np.integer)):
            qs = [int(qindex)]
        else:
            qs = [int(q) for q in qindex]
            if len(qs) != n:
                raise ValueError(f"{who}: {len(qs)} qindex values for {n} jobs")
            jq = (ctypes.c_uint8 * n)(*[q & 255 for q in qs])
        d = [int(v) for v in deltas]
        z = [int(v) for v in zbin]
        if any(not 0 <= q <= 127 for q in qs) or len(d) != 5 or any(not -15 <= v <= 15 for v in d):
            raise ValueError(f"{who}: qindex {qindex!r} (0..127), deltas {deltas!r} (five of -15..15)")
        if len(z) != 3 or any(abs(v) > QUANT_ZBIN_MAX for v in z):
            raise ValueError(f"{who}: zbin {zbin!r} (zbin_over_quant, zbin_mode_boost, act_zbin_adj, each within +-{QUANT_ZBIN_MAX})")
        if quantizer not in QUANT_QUANTIZERS or stage not in COEF_STAGES:
            raise ValueError(f"{who}: quantizer {quantizer!r} ({', '.join(QUANT_QUANTIZERS)}), stage {stage!r} ({', '.join(COEF_STAGES)})")
        if rdmult is None or rddiv is None:
            if len(set(qs)) > 1:
                raise ValueError(f"{who}: rdmult and rddiv must be given with different qindex values: one pair serves every job")
            m0, d0 = intra_rd(qs[0], d[0], z[0])
            rdmult, rddiv = (m0 if rdmult is None else rdmult), (d0 if rddiv is None else rddiv)
        if mbmode_cost is None or bmode_cost is None:
            mc, bc = intra_costs()
            mbmode_cost, bmode_cost = (mc if mbmode_cost is None else mbmode_cost), (bc if bmode_cost is None else bmode_cost)
        mc, bc = [int(v) for v in mbmode_cost], [int(v) for v in np.asarray(bmode_cost).ravel()]
        if not (0 <= int(rdmult) <= 1000 and 1 <= int(rddiv) <= 100 and 0 <= int(bmode_last) <= 9 and len(mc) == 5 and len(bc) == 1000 and
                all(0 <= v <= 65535 for v in mc + bc)):
            raise ValueError(f"{who}: rdmult {rdmult} (0..1000), rddiv {rddiv} (1..100), bmode_last {bmode_last} (0..9), mbmode_cost [5] and "
                             "bmode_cost [10, 10, 10] of 0..65535")
        p = IntraParams()
        p.q = QuantParams(qs[0], (c_int * 5)(*d), QUANT_QUANTIZERS[quantizer], 0, COEF_STAGES[stage], z[0], z[1], z[2], 0, jq)
        p.rdmult, p.rddiv, p.bmode_last, p.flags, p.planes = int(rdmult), int(rddiv), int(bmode_last), 0 if bpred else INTRA_NO_BPRED, mask or 0
        p.cost.mbmode_cost[:] = mc
        ctypes.memmove(p.cost.bmode_cost, (c_int * 1000)(*bc), 4000)
        arr = (c_int * n)(*fbs)
        rows, cols = self.g.aligned_h // 16, self.g.aligned_w // 16
        shapes = {"coef": ("int16", (n, rows, cols, 25, 16)), "eob": ("uint8", (n, rows, cols, 32)),
                  "stats": ("int32", (n, bin(mask or 0).count("1"), rows, cols)),
                  "rec": ("uint8", (n, int(self.L.vp8hip_i420_size(self.width, self.height)))), "modes": ("uint8", (n, rows, cols, 32))}
        order = ("coef", "eob", "stats", "rec", "modes")
        names = [k for k in order if k in want]
        outs = [("out_" + k, given[k], shapes[k][0], shapes[k][1]) for k in names]

        def call(*args):
            a = dict(zip(names, zip(args[0::2], args[1::2])))
            flat = [v for k in order for v in a.get(k, (None, 0))]
            return self.L.vp8hip_frames_intra_async(self.h, arr, n, ctypes.byref(p), *flat)
        made = self._to_torch(who, outs, call, "vp8hip_frames_intra_async")
        return dict(zip(names, made))

    def _pack_bound_of(self, name, log2_parts):
        """vp8hip_<name>(log2_parts) for the context, ValueError where it gives 0"""
        size = int(getattr(self.L, "vp8hip_" + name)(self.h, int(log2_parts)))
        if not size:
            raise ValueError(f"{name}: log2_parts {log2_parts} (0..3) of a configured context")
        return size

    def _pack_inputs(self, who, coef, side, qindex, deltas, fields, key=False):
        """the inputs the three pack calls check alike, in their order: coef; a key frame's modes (`side`); the parameters; an inter
        frame's mv (`side`, or None).  -> (torch, dev, n, p, jq -- to be kept alive --, side's pointer, side's stride in bytes)"""
        torch, dev = self._torch_device(who)
        rows, cols = self.g.aligned_h // 16, self.g.aligned_w // 16
        if not hasattr(coef, "shape") or len(coef.shape) != 5 or not self._dense(coef, torch.int16, (coef.shape[0], rows, cols, 25, 16), dev) or not coef.shape[0]:
            raise ValueError(f"{who}: coef must be an int16 tensor {['n', rows, cols, 25, 16]}, each job dense, on {dev}")
        n = int(coef.shape[0])
        if key and (not hasattr(side, "shape") or not self._dense(side, torch.uint8, (n, rows, cols, 32), dev)):
            raise ValueError(f"{who}: modes must be a uint8 tensor {[n, rows, cols, 32]}, each job dense, on {dev}")
        p, jq = _pack_params(who, qindex, deltas, fields, n, key=key)
        if side is None:
            return torch, dev, n, p, jq, None, 0
        if not key and not self._dense(side, torch.int16, (n, 2, rows, cols), dev):
            raise ValueError(f"{who}: mv must be an int16 tensor {[n, 2, rows, cols]}, each job dense, on {dev}")
        return torch, dev, n, p, jq, c_void_p(side.data_ptr()), side.stride(0) * side.element_size()

    def _pack_cap(self, who, cap, out_data, bound_fn, p):
        """`cap` or its default -- out_data's second dimension, else the bound --, checked"""
        if cap is None:
            cap = int(out_data.shape[1]) if out_data is not None and len(out_data.shape) == 2 else int(bound_fn(self.h, p.log2_parts))
        cap = int(cap)
        if cap < 16 or cap % 16:
            raise ValueError(f"{who}: cap {cap} (a multiple of 16; log2_parts 0..3)")
        return cap

    def _pack_info16(self, who, out_info, torch, dev, n):
        """a given out_info of frames_pack and frames_pack_key, checked (after `cap`, as the wrappers always did)"""
        if out_info is not None and not (self._dense(out_info, torch.int32, (n, 16), dev) and out_info.is_contiguous()):
            raise ValueError(f"{who}: out_info must be a contiguous int32 tensor {[n, 16]} on {dev}")

    def pack_bound(self, log2_parts=0):
        """a `cap` that always suffices for a frame of frames_pack at the context's size (vp8hip_pack_bound): a multiple of 16, and
        loose -- real frames are a hundredth of it"""
        return self._pack_bound_of("pack_bound", log2_parts)

    def frames_pack(self, mv, coef, qindex=40, deltas=(0, 0, 0, 0, 0), cap=None, out_data=None, out_info=None, **fields):
        """Compressed VP8 inter frames from frames_quant's levels and vectors on the context's device (vp8hip_frames_pack_async;
        include/vp8hip.h has the definition): job i's frame -- tag, first partition, size table, 1 << log2_parts token partitions
        -- from mv[i] and coef[i], byte for byte what the test suite's stream writer writes for the same content.  `mv`:
        frames_subpel's torch.int16 tensor [n, 2, mb_rows, mb_cols] as it stands, None: (0, 0); `coef`: frames_quant's "levels"
        tensor [n, mb_rows, mb_cols, 25, 16] (torch.int16, stride(0) a multiple of 16 bytes).  `qindex`: 0..127, or a sequence of
        n; `deltas` as frames_quant's; fields: PACK_DEFAULTS' names (ref_frame 1..3, log2_parts 0..3, the probabilities 1..255
        ...).  `cap`: the most bytes a frame may take, a multiple of 16 (default: out_data's second dimension where that is given, else
        pack_bound(log2_parts), which at large sizes
        makes the call's scratch large: pass what the content needs and watch PACK_OVERFLOW).  Returns (data, info): torch.uint8
        [n, cap] and torch.int32 [n, 16] -- [0] the status (PACK_* bits), [1] the frame's bytes (0 where the status forbids),
        [2] the first partition's, [3..10] the token partitions', [11] skipped macroblocks, [12..15] ZEROMV, NEARESTMV, NEARMV,
        NEWMV macroblocks; pack_frames gives the frames as bytes.  out_data: a uint8 tensor [n, cap], pointer and stride(0)
        multiples of 16; out_info: int32 [n, 16], contiguous.  Stream ordering, the `import torch` first rule and the remark on
        record_stream: as frames_scaled."""
        who = "frames_pack"
        torch, dev, n, p, jq, mptr, mstride = self._pack_inputs(who, coef, mv, qindex, deltas, fields)
        cap = self._pack_cap(who, cap, out_data, self.L.vp8hip_pack_bound, p)
        self._pack_info16(who, out_info, torch, dev, n)
        outs = [("out_data", out_data, "uint8", (n, cap)), ("out_info", out_info, "int32", (n, 16))]
        made = self._to_torch(who, outs, lambda dp, ds, ip, istride: self.L.vp8hip_frames_pack_async(
            self.h, n, ctypes.byref(p), mptr, mstride, c_void_p(coef.data_ptr()), coef.stride(0) * 2, dp, ds, cap, ip), "vp8hip_frames_pack_async")
        del jq
        return made[0], made[1]

    def pack_key_bound(self, log2_parts=0):
        """a `cap` that always suffices for a frame of frames_pack_key at the context's size (vp8hip_pack_key_bound)"""
        return self._pack_bound_of("pack_key_bound", log2_parts)

    def frames_pack_key(self, modes, coef, qindex=40, deltas=(0, 0, 0, 0, 0), cap=None, out_data=None, out_info=None, **fields):
        """Compressed VP8 key frames from frames_intra's modes and levels on the context's device (vp8hip_frames_pack_key_async;
        include/vp8hip.h has the definition): job i's frame -- tag, start code and size, first partition, size table, 1 <<
        log2_parts token partitions -- from modes[i] and coef[i], byte for byte what the test suite's stream writer writes for the
        same content.  `modes`: frames_intra's "modes" tensor [n, mb_rows, mb_cols, 32] (torch.uint8, stride(0) a multiple of 4) --
        [0] the y mode, [1] the uv mode, [4..19] the sub-block modes, read where the y mode is B_PRED; `coef`: its "coef" tensor of
        levels [n, mb_rows, mb_cols, 25, 16] (torch.int16, stride(0) a multiple of 16 bytes).  qindex, deltas, cap (default:
        out_data's second dimension, else pack_key_bound(log2_parts)), out_data, out_info: as frames_pack; fields:
        PACK_KEY_DEFAULTS' names.  Returns (data, info): torch.uint8 [n, cap] and torch.int32 [n, 16] -- [0] the status
        (PACK_OVERFLOW, PACK_BAD_LEVEL, PACK_BAD_MODE), [1] the frame's bytes (0 where the status forbids), [2] the first
        partition's, [3..10] the token partitions', [11] skipped macroblocks, [12] B_PRED macroblocks; pack_frames gives the frames
        as bytes.  Stream ordering, the `import torch` first rule and the remark on record_stream: as frames_scaled."""
        who = "frames_pack_key"
        torch, dev, n, p, jq, modes_ptr, modes_stride = self._pack_inputs(who, coef, modes, qindex, deltas, fields, key=True)
        cap = self._pack_cap(who, cap, out_data, self.L.vp8hip_pack_key_bound, p)
        self._pack_info16(who, out_info, torch, dev, n)
        outs = [("out_data", out_data, "uint8", (n, cap)), ("out_info", out_info, "int32", (n, 16))]
        made = self._to_torch(who, outs, lambda dp, ds, ip, istride: self.L.vp8hip_frames_pack_key_async(
            self.h, n, ctypes.byref(p), modes_ptr, modes_stride, c_void_p(coef.data_ptr()), coef.stride(0) * 2, dp, ds, cap, ip),
            "vp8hip_frames_pack_key_async")
        del jq
        return made[0], made[1]

    def pack_adapt_bound(self, log2_parts=0):
        """a `cap` that always suffices for a frame of frames_pack_adapt at the context's size (vp8hip_pack_adapt_bound)"""
        return self._pack_bound_of("pack_adapt_bound", log2_parts)

    def frames_pack_adapt(self, mv, coef, qindex=40, deltas=(0, 0, 0, 0, 0), cap=None, flags=ADAPT_ALL, refresh_entropy_probs=1, probs_in=None,
                          counts=False, probs=False, out_data=None, out_info=None, out_counts=None, out_probs=None, **fields):
        """frames_pack with probabilities fitted to each frame's own counts by the reference encoder's rules and coded into its
        header where an update pays for itself (vp8hip_frames_pack_adapt_async; include/vp8hip.h has the definition).  mv, coef,
        qindex, deltas, cap (default: pack_adapt_bound), out_data and the fields: as frames_pack.  `flags`: ADAPT_COEF | ADAPT_MV |
        ADAPT_SKIP | ADAPT_REF, what is fitted; the rest keeps the baseline (for skip and the reference probabilities: the
        fields' values) and codes no update.  `refresh_entropy_probs`: the header bit.  `probs_in`: the baseline set(s), a
        torch.uint8 tensor [1104] (one for all jobs) or [n, 1104] (stride(0) and pointer multiples of 16) on the device, None:
        the defaults (pack_probs_default).  Returns (data, info, counts, probs): torch.uint8 [n, cap]; torch.int32 [n, 32] --
        [0..15] as frames_pack's, [16] coefficient probabilities updated, [17] vector probabilities updated, [18] the
        prob_skip_false coded, [19] the estimated saving in bits, the rest 0 --; with `counts` (or out_counts, int32 [n, 1216],
        contiguous) the token counts [4][8][3][12] and 2 x 32 vector branch counts, else None; with `probs` (or out_probs, uint8
        [n, 1104], contiguous, 16-byte aligned) the effective sets -- the next frame's probs_in where refresh_entropy_probs is 1
        --, else None."""
        who = "frames_pack_adapt"
        torch, dev, n, p, jq, mptr, mstride = self._pack_inputs(who, coef, mv, qindex, deltas, fields)
        a = PackAdapt(int(flags), int(refresh_entropy_probs), None, 0)
        if probs_in is not None:
            one = hasattr(probs_in, "shape") and len(probs_in.shape) == 1
            shape = (PACK_PROBS_BYTES,) if one else (n, PACK_PROBS_BYTES)
            if not hasattr(probs_in, "shape") or tuple(probs_in.shape) != shape or probs_in.dtype != torch.uint8 or probs_in.device != dev or probs_in.stride(-1) != 1:
                raise ValueError(f"{who}: probs_in must be a uint8 tensor [{PACK_PROBS_BYTES}] or {[n, PACK_PROBS_BYTES]}, each set dense, on {dev}")
            a.probs_in, a.probs_in_stride = probs_in.data_ptr(), 0 if one else probs_in.stride(0)
        cap = self._pack_cap(who, cap, out_data, self.L.vp8hip_pack_adapt_bound, p)
        outs = [("out_data", out_data, "uint8", (n, cap)), ("out_info", out_info, "int32", (n, 32))]
        if counts or out_counts is not None:
            outs.append(("out_counts", out_counts, "int32", (n, PACK_COUNTS)))
        if probs or out_probs is not None:
            outs.append(("out_probs", out_probs, "uint8", (n, PACK_PROBS_BYTES)))
        for arg, t, _, _ in outs[1:]:
            if t is not None and not t.is_contiguous():
                raise ValueError(f"{who}: {arg} must be contiguous")

        def call(dp, ds, ip, istride, *rest):
            opt = dict(zip([o[0] for o in outs[2:]], rest[0::2]))
            return self.L.vp8hip_frames_pack_adapt_async(self.h, n, ctypes.byref(p), ctypes.byref(a), mptr, mstride, c_void_p(coef.data_ptr()),
                                                         coef.stride(0) * 2, dp, ds, cap, ip, opt.get("out_counts"), opt.get("out_probs"))
        made = dict(zip([o[0] for o in outs], self._to_torch(who, outs, call, "vp8hip_frames_pack_adapt_async")))
        del jq
        return made["out_data"], made["out_info"], made.get("out_counts"), made.get("out_probs")

    def ssim_share(self, n, planes=("y", "u", "v")):
        """how many workgroups share each job of a frames_ssim call of n jobs over `planes` (vp8hip_ssim_share): 1 -- a workgroup
        owns a job and stores its scores -- or more -- the scores are zeroed first and the workgroups add to them.  The results do
        not depend on it."""
        mask = _plane_mask(planes, HIST_PLANES, False)
        return int(self.L.vp8hip_ssim_share(self.h, int(n), mask or 0))

    def trace_residual(self, pool, jobs, width=None, height=None, dtype=None, matrix="bt601", order="rgb", scale=None, out=None):
        """The accumulated residual of `jobs` -- a list of (fb, entry, anchor_fb): the frame buffer that holds a frame, the entry of
        `pool` that holds its trace (frames_trace) and the frame buffer the caller keeps the group's anchor picture in; any order,
        repeats allowed -- as tensors [n, 3, gh, gw] on the context's device (vp8hip_trace_residual_async): the frame's RGB bytes
        minus the anchor's at the position the trace names (clamped to the picture), -255 .. 255, converted with `matrix` and in
        `order` as frames_rgb's "nchw" tensor is, at the display size or under each output's centre at width x height (then the
        tensor lines up with frames_rgb's and trace_flow's at that size).  torch.int16 (the default), torch.float16 or
        torch.float32; float types: float32(float64(a) * scale[c]) with scale = one number or (R, G, B), by colour, float32
        (default 1).  Both frame buffers are read in the form they have; nothing is converted or allocated.  `out`: a tensor of that
        shape and type, each frame dense, stride(0) free.  Stream ordering: as frames_scaled."""
        import torch
        arr, n = self._trace_jobs("trace_residual", jobs, AnchorJob, "(fb, entry, anchor_fb)")
        dst_w, dst_h, gw, gh = self._trace_grid("trace_residual", width, height)
        dtype = torch.int16 if dtype is None else dtype
        dt = _elem_dtype(dtype, _INT16_DTYPES)
        if dt is None or matrix not in RGB_MATRICES or order not in RGB_ORDERS:
            raise ValueError(f"trace_residual: dtype {dtype}, matrix {matrix!r}, order {order!r}")
        if scale is None:
            sc = (1.0, 1.0, 1.0)
        elif isinstance(scale, str):
            raise ValueError(f"trace_residual: scale {scale!r}")
        elif np.ndim(scale) == 0:
            sc = (float(scale),) * 3
        else:
            sc = tuple(float(v) for v in scale)
            if len(sc) != 3:
                raise ValueError(f"trace_residual: scale {scale!r}")
        p = TraceResidualParams(dst_w, dst_h, RGB_MATRICES[matrix], RGB_ORDERS[order], dt)
        for c in range(3):
            p.scale[c] = np.float32(sc[c])
        if not self.L.vp8hip_trace_residual_size(self.h, ctypes.byref(p)):
            raise ValueError(f"trace_residual: grid {gw}x{gh}: refused (sizes 1..16383)")
        _, pptr, pstride, entries = self._trace_pool_args("trace_residual", pool)
        return self._to_torch("trace_residual", [("out", out, _INT16_DTYPES[dt], (n, 3, gh, gw))],
                              lambda arr_out, stride: self.L.vp8hip_trace_residual_async(
                                  self.h, arr, n, ctypes.byref(p), pptr, pstride, entries, arr_out, stride),
                              "vp8hip_trace_residual_async")[0]

    def trace_gather(self, pool, jobs, src, width=None, height=None, filter="nearest", out=None):
        """`src` -- tensors [m, C, sh, sw] a model made of anchor pictures: feature maps of any stride, logits, a label map -- carried
        to later frames along their traces (vp8hip_trace_gather_async).  `jobs`: a list of (entry, k): the entry of `pool` that
        holds a frame's trace (frames_trace) and the source tensor src[k]; any order, repeats allowed.  Returns [n, C, gh, gw] of
        src's type and memory format, at the display size or under each output's centre at width x height: "nearest" the cell
        under the anchor position the trace names (clamped to the picture), the element's bits, for any type of 1, 2 or 4 bytes;
        "bilinear" the four cells around it weighted in 1/256 steps, in single precision, torch.float16 / torch.float32 only,
        within the bound include/vp8hip.h derives.  A contiguous src is read as planar [C][h][w], a channels_last one as
        [h][w][C]; each tensor dense, stride(0) free; anything else is refused.  A src that is both -- one channel, or a grid of
        one cell -- is read as planar, unless `out` is given and is channels_last only.  `out`: a tensor of that shape, type and
        format, each frame dense, stride(0) free, not overlapping src.  Stream ordering: as frames_scaled -- the wait on torch's
        current stream also covers src, which the model has just produced there."""
        torch, dev = self._torch_device("trace_gather")
        arr, n = self._trace_jobs("trace_gather", jobs, GatherJob, "(entry, source tensor)")
        if filter not in GATHER_FILTERS:
            raise ValueError(f"trace_gather: filter {filter!r}")
        if not (torch.is_tensor(src) and src.dim() == 4 and src.shape[0] >= 1 and src.device == dev):
            raise ValueError(f"trace_gather: src must be a tensor [m, C, sh, sw] on {dev}")
        m, C, sh, sw = (int(v) for v in src.shape)

        def planar(t):
            return t[0].is_contiguous()

        def channels_last(t):
            return t[0].permute(1, 2, 0).is_contiguous()
        if not planar(src) and not channels_last(src):
            raise ValueError("trace_gather: src must be contiguous (planar) or channels_last, each tensor dense")
        layout = "planar" if planar(src) else "channels_last"
        if planar(src) and channels_last(src) and torch.is_tensor(out) and out.dim() == 4 and out.shape[0] and not planar(out):
            layout = "channels_last"
        is_fmt = planar if layout == "planar" else channels_last
        es = src.element_size()
        if es not in (1, 2, 4) or (filter == "bilinear" and src.dtype not in (torch.float16, torch.float32)):
            raise ValueError(f"trace_gather: {src.dtype} with filter {filter!r} (any type of 1, 2 or 4 bytes; bilinear: float16 / float32)")
        dst_w, dst_h, gw, gh = self._trace_grid("trace_gather", width, height)
        p = TraceGatherParams(dst_w, dst_h, sw, sh, C, es, GATHER_LAYOUTS[layout], GATHER_FILTERS[filter])
        if not self.L.vp8hip_trace_gather_size(self.h, ctypes.byref(p)):
            raise ValueError(f"trace_gather: grid {gw}x{gh}, source [{C}, {sh}, {sw}]: refused (sizes 1..16383, channels 1..4096)")
        _, pptr, pstride, entries = self._trace_pool_args("trace_gather", pool)
        if out is None:
            out = torch.empty((n, C, gh, gw), dtype=src.dtype, device=dev,
                              memory_format=torch.contiguous_format if layout == "planar" else torch.channels_last)
        src_stride = (src.stride(0) if m > 1 else C * sh * sw) * es      # (of one tensor torch keeps any stride(0): the dense size)

        def fits(t, dtype, shape, d):
            return t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.device == d and (shape[0] == 0 or is_fmt(t))
        return self._to_torch("trace_gather", [("out", out, str(src.dtype).split(".")[-1], (n, C, gh, gw))],
                              lambda arr_out, stride: self.L.vp8hip_trace_gather_async(
                                  self.h, arr, n, ctypes.byref(p), pptr, pstride, entries, c_void_p(src.data_ptr()), src_stride, m,
                                  arr_out, stride),
                              "vp8hip_trace_gather_async", ok=fits, how=f"{layout}, each frame dense")[0]

    def rgb_scratch_bytes(self):
        """device bytes of frames_rgb's scratch (vp8hip_rgb_scratch_bytes): a chunk of scaled frames as packed I420; a cache"""
        return int(self.L.vp8hip_rgb_scratch_bytes(self.h))

    def release_staging(self):
        """vp8hip_release_staging: free the packed staging of downloads and frames_rgb's scratch now"""
        self._chk(self.L.vp8hip_release_staging(self.h), "vp8hip_release_staging")

    def frames_to_raster(self, first_fb, count):
        """Ask for the raster form of frame buffers a large launch left as tiles (vp8hip_frames_to_raster; asynchronous)."""
        self._chk(self.L.vp8hip_frames_to_raster(self.h, first_fb, count), "vp8hip_frames_to_raster")

    def upload_frame(self, fb, buf):
        assert buf.nbytes == self.g.frame_size
        self._chk(self.L.vp8hip_frame_upload(self.h, fb, buf.ctypes.data), "upload")

    def postproc(self, src_fb, dst_fb, tmp_fb, flags, flimit=0, mb_flimit=0, rv_offset=0, noise=None, noise_clamp=0, noise_rows=None):
        """Output-side filters of vp8/common/postproc.c from frame buffer src_fb into dst_fb (include/vp8hip.h).  noise: int8
        array of 3072, noise_rows: uint8 array, one phase per row of the aligned height."""
        pp = PostprocParams(flags, flimit, mb_flimit, rv_offset, noise_clamp,
                            ctypes.cast(load_host().vp8t_pp_rv, c_void_p) if flags & PP_DEMACROBLOCK else None,
                            noise.ctypes.data if noise is not None else None,
                            noise_rows.ctypes.data if noise_rows is not None else None)
        self._chk(self.L.vp8hip_postproc(self.h, src_fb, dst_fb, tmp_fb, ctypes.byref(pp)), "postproc")

    def entropy_decode(self, first_slot, frames, datas):
        """vp8hip_entropy_decode: frames = EntropyFrame list (from Parser.export_entropy), datas = the frames' bytes; slot
        first_slot + i receives frame i's IR.  Returns the per-frame status words (synchronises)."""
        n = len(frames)
        arr = (EntropyFrame * n)()
        off = 0
        for i, (f, d) in enumerate(zip(frames, datas)):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(f), ctypes.sizeof(EntropyFrame))
            arr[i].data_off = off
            off += len(d)
        blob = b"".join(datas)
        self._chk(self.L.vp8hip_entropy_decode(self.h, first_slot, n, ctypes.byref(arr), blob, len(blob)), "entropy_decode")
        st = np.zeros(n, np.uint32)
        self._chk(self.L.vp8hip_entropy_status(self.h, n, st.ctypes.data), "entropy_status")
        return st

    def mvs_fetch(self, slot):
        """The slot's motion vectors as they stand on the device: int16[n * 16, 2] (row, col)."""
        mv = np.zeros((self.g_mbs() * 16, 2), np.int16)
        self._chk(self.L.vp8hip_ir_fetch_mvs(self.h, slot, mv.ctypes.data), "ir_fetch_mvs")
        return mv

    def ir_fetch(self, slot):
        """The slot's IR as it stands on the device: (mbs uint8[n,64], coef int16[n,400])."""
        n = self.g_mbs()
        mbs = np.zeros((n, 64), np.uint8)
        coef = np.zeros((n, 400), np.int16)
        self._chk(self.L.vp8hip_ir_fetch(self.h, slot, mbs.ctypes.data, coef.ctypes.data), "ir_fetch")
        return mbs, coef

    def mfqe(self, show_fb, prev_fb, dst_fb, mb_class, qcurr, qprev):
        """vp8_multiframe_quality_enhance (postproc.c:802-900; include/vp8hip.h): mb_class a uint8 array, a byte per macroblock."""
        mb_class = np.ascontiguousarray(mb_class, np.uint8)
        assert mb_class.size == self.g_mbs()
        self._chk(self.L.vp8hip_mfqe(self.h, show_fb, prev_fb, dst_fb, mb_class.ctypes.data, qcurr, qprev), "mfqe")

    def visualize(self, fb, slot, flags, ref_frame_mask=0, mb_modes_mask=0, b_modes_mask=0, mv_mask=0, frame_info=None,
                  rate_info=None):
        """The decoder's debug overlays (VP8D_DEBUG_* flags, the four VP8_SET_DBG_* masks) drawn into frame buffer fb in place from
        the macroblocks of IR slot `slot` (include/vp8hip.h); the strings are str or None."""
        v = VisParams(flags, ref_frame_mask, mb_modes_mask, b_modes_mask, mv_mask,
                      frame_info.encode("latin-1") if frame_info is not None else None,
                      rate_info.encode("latin-1") if rate_info is not None else None)
        self._chk(self.L.vp8hip_visualize(self.h, fb, slot, ctypes.byref(v)), "visualize")

    def g_mbs(self):
        return (self.g.aligned_w // 16) * (self.g.aligned_h // 16)


def decode_ivf_gpu(path, device=-1, stages=STAGE_ALL):
    """Decode a whole IVF on the GPU, frame by frame (the latency path): list of per-shown-frame MD5s."""
    w, h, frames = read_ivf(path)
    parser, ctx = Parser(), Vp8Hip(device)
    out = []
    try:
        for data in frames:
            hdr, changed = parser.begin(data)
            if changed:
                ctx.configure(hdr.width, hdr.height, 4, 1)
            _, pm, pc, pv = ctx.ir_map(0)
            ph = ctx.ir_map(0)[0]
            parser.decode_mbs(pm, pc, pv)
            ctypes.memmove(ph, ctypes.byref(hdr), 64)
            ctx.upload(0)
            r = parser.refs
            ctx.decode([(0, r.new_idx, (r.lst_idx, r.gld_idx, r.alt_idx))], stages)
            parser.swap(hdr)
            if hdr.show_frame:
                out.append(planes_md5(*ctx.download_planes(parser.refs.show_idx)))
            else:
                ctx.sync()
    finally:
        ctx.close()
        parser.close()
    return out
