"""What the GPU tests of the calls that hand something to a device consumer as tensors share (test_gpu_scale.py, test_gpu_rgb.py,
test_gpu_side.py, test_gpu_residual.py, test_gpu_coef.py, the trace tests through trace_testlib.py, and the three that read picture
pairs, test_gpu_hist.py, test_gpu_ssim.py and test_gpu_motion.py): frames into frame buffers and into IR slots, pictures into frame
buffer images, bit patterns, guarded destinations, the destinations every call refuses, the writers that come after a call and the
decode a call over picture pairs is ordered against.  torch is imported here before anything loads libvp8hip.so: one HIP runtime
per process."""
import ctypes

import torch
import numpy as np

from vp8_testlib import ivf_path
import scale_reference as SC

TORCH_DTYPE = {"u8": torch.uint8, "i16": torch.int16, "f16": torch.float16, "f32": torch.float32}
BITS = {"u8": np.uint8, "i16": np.uint16, "f16": np.uint16, "f32": np.uint32}


def bits(a, dtype):
    """numpy array -> its bit pattern (floats compared as integers: bit for bit, signed zeros included)"""
    return np.ascontiguousarray(a).view(BITS[dtype])


def hip_range(ptr):
    """(base, size) of the HIP allocation holding ptr, through the HIP runtime torch and the library share"""
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMemGetAddressRange.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
    base, size = ctypes.c_void_p(), ctypes.c_size_t()
    assert hip.hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(ptr)) == 0
    return base.value, size.value


def equal_on_device(out, refs, which, dtype):
    """frame i of `out` against refs[which[i]] (numpy), compared on the device as bit patterns; -> indices of differing frames"""
    view = {"u8": torch.uint8, "i16": torch.int16, "f16": torch.int16, "f32": torch.int32}[dtype]
    np_view = {"u8": np.uint8, "i16": np.int16, "f16": np.int16, "f32": np.int32}[dtype]
    t = torch.from_numpy(np.stack([np.ascontiguousarray(r).view(np_view) for r in refs])).to(out.device)
    idx = torch.as_tensor(which, device=out.device)
    step = max(1, min(512, (1 << 28) // (t[0].numel() * t.element_size())))      # (frames gathered at a time: a quarter of a gigabyte)
    bad = []
    for a in range(0, len(which), step):
        diff = (out[a:a + step].view(view) != t[idx[a:a + step]]).flatten(1).any(1)
        bad += [a + int(i) for i in diff.nonzero().flatten().tolist()]
    return bad


def decode_stream(P, name, form, monkeypatch, extra_fb=0):
    """every frame of a fixture into a frame buffer of its own, one launch per frame; -> (ctx, frame buffers of the shown frames)"""
    monkeypatch.setenv("VP8HIP_RECON", "simt" if form == "tiles" else "wave")
    w, h, frames = P.read_ivf(ivf_path(name))
    nf = len(frames)
    ctx = P.Vp8Hip(0)
    ctx.configure(w, h, nf + 1 + extra_fb, 1)
    parser = P.Parser()
    phys, shown = {}, []
    try:
        for i, data in enumerate(frames):
            hdr, _ = ctx.parse_into_slot_compact(parser, data, 0)
            r = parser.refs
            ctx.decode([(0, i, tuple(phys.get(k, nf) for k in (r.lst_idx, r.gld_idx, r.alt_idx)))], P.STAGE_ALL)
            ctx.sync()
            new = r.new_idx
            parser.swap(hdr)
            phys[new] = i
            if hdr.show_frame:
                shown.append(phys[parser.refs.show_idx])
    finally:
        parser.close()
    return ctx, shown


def large_launch(P, ctx, name, n, monkeypatch):
    """n frame buffers written as tiles by one launch: the fixture's key frames, repeated; -> how many the fixture has"""
    monkeypatch.setenv("VP8HIP_RECON", "simt")
    w, h, frames = P.read_ivf(ivf_path(name))
    ctx.configure(w, h, n + 2, n)
    parser = P.Parser()
    for i, data in enumerate(frames[:n]):
        ctx.sync()
        hdr, _ = ctx.parse_into_slot_compact(parser, data, i)
        parser.swap(hdr)
    parser.close()
    for i in range(len(frames), n):
        ctx.ir_copy(i, i % len(frames))
    ctx.decode([(i, i, None) for i in range(n)], P.STAGE_ALL)
    return len(frames)


def picture_into(buf, g, planes):
    """display-size planes (y, u, v) into the frame buffer image `buf`; what lies around them stays"""
    for view, p in zip(SC.planes(buf, g), planes):
        view[:p.shape[0], :p.shape[1]] = p
    return buf


def two_key_frames_queued(P):
    """-> (ctx, parser): the two key frames of kf_640x360 in slots 0 and 1 of a context of two frame buffers; frame 1 is decoded
    into frame buffer 1 and waited for, the decode of frame 0 into frame buffer 0 is queued and not waited for"""
    w, h, frames = P.read_ivf(ivf_path("kf_640x360"))
    ctx = P.Vp8Hip(0)
    parser = P.Parser()
    try:
        ctx.configure(w, h, 2, 2)
        for i in range(2):
            hdr, _ = ctx.parse_into_slot_compact(parser, frames[i], i)
            parser.swap(hdr)
        ctx.decode([(1, 1, None)], P.STAGE_ALL)
        ctx.sync()
        ctx.decode([(0, 0, None)], P.STAGE_ALL)
    except BaseException:
        parser.close()
        ctx.close()
        raise
    return ctx, parser


class Producer:
    """a stream's frames, one after the other, into a slot of a context: by the host parser (parse_into_slot_compact) or by the
    device's entropy decoder (also on a context whose slots take their blocks from a pool)"""

    def __init__(self, P, name, how, nslots=1):
        self.P, self.how = P, how
        self.w, self.h, self.frames = P.read_ivf(ivf_path(name))
        self.ctx = P.Vp8Hip(0)
        w, h = self.w, self.h
        if how == "pooled":
            cols = (w + 15) // 16
            nmb = cols * ((h + 15) // 16)
            self.ctx.configure_pooled(w, h, 1, nslots, nslots * nmb * 24 * 32 + (nslots + 3) * 4 * cols * 24 * 32)
        else:
            self.ctx.configure(w, h, 1, nslots)
        self.parser = P.Parser()
        if how != "host":
            self.parser.set_device_segmap(True)

    def put(self, i, slot=0):
        """frame i (in stream order) into `slot`; -> the header the slot now has"""
        ctx, data = self.ctx, self.frames[i]
        if self.how == "host":
            ctx.sync()                                  # (the staging may still be on its way)
            hdr, _ = ctx.parse_into_slot_compact(self.parser, data, slot)
            self.parser.swap(hdr)
            return hdr
        hdr, _ = self.parser.begin(data)
        ef = self.parser.export_entropy()
        assert ef is not None
        if self.how == "pooled":
            ctx.pool_reset()
        assert not ctx.entropy_decode(slot, [ef], [data]).any()
        self.parser.swap(hdr)
        return ef.hdr

    def close(self):
        self.parser.close()
        self.ctx.close()


def later_writers_producer(P, name, how, n):
    """-> (prod, hdrs, staged): frames 0 .. n - 1 of a stream in slots 0 .. n - 1 (hdrs: their headers), ready for
    write_later_frames; "copy": frames n .. 2n - 1 wait in slots n .. 2n - 1 (staged: their headers)"""
    prod = Producer(P, name, "host" if how == "copy" else how, nslots=2 * n)
    hdrs = [prod.put(i, i) for i in range(n)]
    staged = None
    if how == "copy":
        staged = [prod.put(n + i, n + i) for i in range(n)]
        prod.ctx.sync()
    return prod, hdrs, staged


def write_later_frames(P, prod, how, n, staged):
    """frames n .. 2n - 1 into slots 0 .. n - 1 with nothing waited for -- an upload each ("host"), one entropy launch ("entropy"),
    vp8hip_ir_copy from the slots that hold them ("copy") -- right behind a call that reads the slots; -> the headers they now have"""
    ctx = prod.ctx
    if how == "host":
        hdrs = []
        for i in range(n):                              # (no sync: the stagings' earlier uploads have landed, the test's fetches waited)
            hdr, _ = ctx.parse_into_slot_compact(prod.parser, prod.frames[n + i], i)
            prod.parser.swap(hdr)
            hdrs.append(hdr)
        return hdrs
    if how == "copy":
        for i in range(n):
            ctx.ir_copy(i, n + i)
        return staged
    efs = []
    for i in range(n):
        hdr, _ = prod.parser.begin(prod.frames[n + i])
        efs.append(prod.parser.export_entropy())
        prod.parser.swap(hdr)
    arr = (P.EntropyFrame * n)()
    off = 0
    for i, ef in enumerate(efs):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(ef), ctypes.sizeof(P.EntropyFrame))
        arr[i].data_off = off
        off += len(prod.frames[n + i])
    blob = b"".join(prod.frames[n:2 * n])
    ctx._chk(ctx.L.vp8hip_entropy_decode(ctx.h, 0, n, ctypes.byref(arr), blob, len(blob)), "entropy_decode")
    return [ef.hdr for ef in efs]


def guarded(n, size, pad, off, fill=0xA5):
    """-> (big, frames): a device buffer of `fill` bytes and, inside it, n frames of `size` bytes, size + pad apart, the first at
    byte `off`: a uint8 view [n, size] with stride(0) = size + pad; `off` and 64 guard bytes behind the last stride"""
    stride = size + pad
    big = torch.full((n * stride + 2 * off + 64,), fill, dtype=torch.uint8, device="cuda:0")
    return big, big[off:off + n * stride].view(n, stride)[:, :size]


def assert_guards_intact(big, n, size, pad, off, fill=0xA5, what=None):
    """every byte of `big` (guarded) before, between and behind the frames still holds `fill`"""
    a = big.cpu().numpy()
    mask = np.ones(a.size, bool)
    for i in range(n):
        mask[off + i * (size + pad): off + i * (size + pad) + size] = False
    assert (a[mask] == fill).all(), what


def assert_destinations_refused(ctx, run, d, size, es, null=True):
    """The destinations every call refuses with -2, through the test's run(n, dst, stride) -> status, which asks for n of three frames
    of `size` bytes, elements of `es` bytes, in a form that is accepted at d (device memory the test owns, 16-byte aligned, three
    frames and more before the allocation's end): null (not where run() has another destination that would do), a short stride,
    pointer or stride not aligned to the element, page-locked and pageable host memory, past the allocation's end, a span that
    wraps, another device's memory.  Nothing may be enqueued by any of them: the caller checks its memory afterwards."""
    L = ctx.L
    assert d % 16 == 0
    if null:
        assert run(3, None, size) == -2
    assert run(3, d, size - es) == -2
    if es > 1:
        assert run(3, d + es // 2, size) == -2
        assert run(3, d, size + es // 2) == -2
        assert run(3, d + es // 2, size + es) == -2
    L.vp8hip_host_alloc.restype = ctypes.c_void_p
    L.vp8hip_host_alloc.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    L.vp8hip_host_free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    host = L.vp8hip_host_alloc(ctx.h, 3 * size)
    try:
        assert run(3, host, size) == -2
    finally:
        L.vp8hip_host_free(ctx.h, host)
    pageable = np.zeros(3 * size, np.uint8)
    assert run(3, pageable.ctypes.data, size) == -2
    base, asize = hip_range(d)
    end = base + asize
    assert run(1, end - size + es, size) == -2              # one element past the allocation
    assert run(3, end - 3 * size, size + es) == -2          # the stride carries the last frame past it
    assert run(3, d, 1 << 62) == -2                         # spans that wrap
    assert run(3, d, (1 << 63) + 8) == -2
    if torch.cuda.device_count() > 1:
        other = torch.empty(3 * size, dtype=torch.uint8, device="cuda:1")
        assert run(3, other.data_ptr(), size) == -2
