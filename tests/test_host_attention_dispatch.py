"""Host only: the shape dispatch of csrc/attention.hip (fmi_attention_fwd_waves, fmi_attention_bwd_structure, the *_uses_pieces
predicates), the image sizes, and the refusals of the four entry points -- all pure host arithmetic that returns before the first HIP
call, so none of this needs (or touches) a GPU."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED = 0, 1, 2

TS = (32, 96, 128, 160, 256, 384, 512, 640, 1024, 4096, 16384)
VALUES = ((64, 0), (32, 32), (128, 0), (32, 96), (96, 32), (256, 0), (128, 128), (512, 0))   # (C1, C2), whole 32s
DS = (16, 32, 48, 64)


@pytest.fixture(scope="module")
def c():
    from face_mask_inpaint_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfmi_hip.so not built")
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for table in (_lib.SIGNATURES, _lib.PREDICATES):
        for name, argtypes in table.items():
            if "attention" in name:
                getattr(cdll, name).argtypes = argtypes
                getattr(cdll, name).restype = ctypes.c_int
    return cdll


def _waves(n, t):
    if t % 256 == 0 and (t // 256) * n >= 256:
        return 8
    return 2 if (t // 128) * n < 256 else 4


def _structure(n, t):
    return 2 if t % 128 == 0 and (t // 128) * n >= 128 else 1


def _ns(t):
    """batch sizes around every threshold of this T, and the ends of the accepted range"""
    ns = {1, 2, 3, 8, 65535}
    for per, need in ((t // 256, 256), (t // 128, 256), (t // 128, 128)):
        if per:
            edge = -(-need // per)
            ns.update((edge - 1, edge, edge + 1))
    return sorted(n for n in ns if 1 <= n <= 65535)


def test_predicates_are_declared():
    import re

    from face_mask_inpaint_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmi_hip.h")).read(), flags=re.S)
    for name in ("fmi_attention_fwd_waves", "fmi_attention_bwd_structure"):
        assert re.search(r"\bint\s+%s\s*\(\s*int\s+N\s*,\s*int\s+T\s*\)" % name, hdr), name
        assert len(_lib.PREDICATES[name]) == 2


def test_dispatch_predicates_follow_the_rules(c):
    """forward: 8 waves if T % 256 == 0 and (T/256) N >= 256, else 2 if (T/128) N < 256, else 4; backward: the second structure if
    T % 128 == 0 and (T/128) N >= 128; the images where that gives 8 / 2 and D in {32, 64}, (C1 + C2) / 32 in {4, 8}"""
    seen = set()
    for t in TS:
        for n in _ns(t):
            w, s = c.fmi_attention_fwd_waves(n, t), c.fmi_attention_bwd_structure(n, t)
            assert (w, s) == (_waves(n, t), _structure(n, t)), (n, t, w, s)
            seen.add((w, s))
            for d in DS:
                for c1, c2 in VALUES:
                    inst = d in (32, 64) and (c1 + c2) // 32 in (4, 8)
                    assert c.fmi_attention_fwd_uses_pieces(n, t, d, c1, c2) == int(w == 8 and inst), (n, t, d, c1, c2)
                    assert c.fmi_attention_bwd_uses_pieces(n, t, d, c1, c2) == int(s == 2 and inst), (n, t, d, c1, c2)
    # the grid reaches every cell that exists: 8 waves imply the second structure, and (4, 1) needs T % 128 != 0 (which only the backward takes)
    assert seen == {(2, 1), (2, 2), (4, 1), (4, 2), (8, 2)}
    # the cells the GPU tests rely on
    assert [c.fmi_attention_fwd_waves(n, t) for n, t in ((256, 128), (86, 384), (128, 256), (256, 256), (128, 512), (255, 128), (85, 384))] \
        == [4, 4, 4, 8, 8, 2, 2]
    assert [c.fmi_attention_bwd_structure(n, t) for n, t in ((1, 128), (2, 384), (127, 128), (2, 96), (3, 160), (128, 128))] == [1, 1, 1, 1, 1, 2]


def _kib(x):
    return (x + 1023) // 1024 * 1024


def test_image_sizes_follow_the_documented_layouts(c):
    """N (T/32) BLK with BLK from the layouts: key tile 3*32*(2D+16) + 3*32*(2CT+64), query tile 3*32*2CT + 3*32*192 + 256, each
    rounded up to whole KiB; 0 where the shape has no image (forward: T % 256, backward: T % 128)"""
    nbytes = ctypes.c_int64(-1)
    for t in TS:
        for n in (1, 3, 128, 65535):
            for d in DS:
                for c1, c2 in VALUES:
                    ct = c1 + c2
                    inst = d in (32, 64) and ct // 32 in (4, 8)
                    kblk = _kib(3 * 32 * (2 * d + 16) + 3 * 32 * (2 * ct + 64))
                    qblk = _kib(3 * 32 * 2 * ct + 3 * 32 * 192 + 256)
                    assert c.fmi_attention_fwd_image_bytes(n, t, d, c1, c2, ctypes.byref(nbytes)) == OK
                    assert nbytes.value == (n * (t // 32) * kblk if inst and t % 256 == 0 else 0), (n, t, d, c1, c2)
                    assert c.fmi_attention_bwd_image_bytes(n, t, d, c1, c2, ctypes.byref(nbytes)) == OK
                    assert nbytes.value == (n * (t // 32) * qblk if inst and t % 128 == 0 else 0), (n, t, d, c1, c2)
    assert c.fmi_attention_fwd_image_bytes(2, 256, 64, 48, 80, ctypes.byref(nbytes)) == OK and nbytes.value == 0   # C1 % 32
    assert c.fmi_attention_fwd_image_bytes(2, 256, 64, 128, 0, None) == BAD_ARG
    assert c.fmi_attention_bwd_image_bytes(0, 256, 64, 128, 0, ctypes.byref(nbytes)) == BAD_ARG


# ---- refusals.  Read off the entry points (csrc/attention.hip): each of the four checks pointers, then the shape, then alignment and
# the image size, and only then makes its first HIP call (hipGetDevice / hipFuncSetAttribute in the launch macros, the delta pass of the
# backward), so each call below returns from host code.  The buffers are host memory and are never dereferenced.
class _Entry:
    """one entry point: argument names in order, and which of them are checked for 16-byte alignment"""

    def __init__(self, name, names, aligned, optional=()):
        self.name, self.names, self.aligned, self.optional = name, names, aligned, optional

    def call(self, c, p, shape, **over):
        n, t, d, c1, c2 = shape
        args = []
        for a in self.names:
            if a in over:
                args.append(over[a])
            elif a == "image_bytes":
                nbytes = ctypes.c_int64(0)
                which = "fwd" if "fwd" in self.name else "bwd"
                getattr(c, f"fmi_attention_{which}_image_bytes")(n, t, d, c1, c2, ctypes.byref(nbytes))
                args.append(nbytes.value)
            else:
                args.append(None if (a.endswith("2") and c2 == 0) else p)
        return getattr(c, self.name)(*args, n, t, d, c1, c2, None)


ENTRIES = [
    _Entry("fmi_attention_fwd_f32", ["q", "v1", "v2", "o1", "o2", "lse"], ["q", "v1", "v2", "o1", "o2"], optional=("lse",)),
    _Entry("fmi_attention_fwd_pieces_f32", ["q", "v1", "v2", "image", "image_bytes", "o1", "o2", "lse"], ["q", "v1", "v2", "o1", "o2", "image"],
           optional=("lse",)),
    _Entry("fmi_attention_bwd_f32", ["q", "v1", "v2", "o1", "o2", "go1", "go2", "lse", "delta", "gv1", "gv2", "gq"],
           ["q", "v1", "v2", "go1", "go2", "gv1", "gv2"]),
    _Entry("fmi_attention_bwd_pieces_f32", ["q", "v1", "v2", "o1", "o2", "go1", "go2", "lse", "delta", "image", "image_bytes", "gv1", "gv2", "gq"],
           ["q", "v1", "v2", "go1", "go2", "gv1", "gv2", "image"]),
]
GOOD = (2, 256, 64, 128, 128)   # accepted by all four


@pytest.mark.parametrize("e", ENTRIES, ids=lambda e: e.name)
def test_refusals_come_back_as_status_codes(c, e):
    """one fault at a time on an otherwise accepted call"""
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 4)
    for a in e.names:
        if a == "image_bytes":
            nbytes = ctypes.c_int64(0)
            getattr(c, "fmi_attention_%s_image_bytes" % ("fwd" if "fwd" in e.name else "bwd"))(*GOOD, ctypes.byref(nbytes))
            assert nbytes.value > 0
            assert e.call(c, p, GOOD, image_bytes=nbytes.value - 1) == BAD_ARG, a
            continue
        if a not in e.optional:
            assert e.call(c, p, GOOD, **{a: None}) == BAD_ARG, a            # a null pointer
        if a in e.aligned:
            assert e.call(c, p, GOOD, **{a: odd}) == BAD_ARG, a             # a pointer off by 4 bytes
    n, t, d, c1, c2 = GOOD
    assert e.call(c, p, (n, 160, d, c1, c2)) == UNSUPPORTED                 # T % 128: the backward takes what the forward produces
    assert e.call(c, p, (n, 48, d, c1, c2)) == UNSUPPORTED
    assert e.call(c, p, (n, t, 48, c1, c2)) == UNSUPPORTED                  # D
    assert e.call(c, p, (n, t, d, 48, 80)) == UNSUPPORTED                   # C1 % 32
    assert e.call(c, p, (n, t, 16, 128, 128)) == UNSUPPORTED                # (D, C / 32) = (16, 8)
    assert e.call(c, p, (n, t, 16, 256, 0)) == UNSUPPORTED
    assert e.call(c, p, (65536, t, d, c1, c2)) == UNSUPPORTED               # N above the grid's y extent
    assert e.call(c, p, (0, t, d, c1, c2)) == BAD_ARG
