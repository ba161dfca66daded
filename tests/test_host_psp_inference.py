"""Host side of the pSp inference harness (face_mask_inpaint_amd/psp_inference.py): the command line against the reference's, the host
tensor2im against the reference's two forms (tests/golden/psp_infer.pt, tools/golden/gen_psp_infer.py), the C boundary of the image-tail
kernels without a GPU, and the refusal to run without one."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the reference's path defaults name its author's machine (data_root) and files it expects in the working directory; here an absent
# path means synthetic input / random initialisation, and the four data sub-paths are joined with data_root in main(), not in get_args()
PATH_ARGS = ("data_root", "src_img_path", "ref_img_path", "mask_path", "identity_file_path", "mask_detector_path", "pt_ckpt_path")
JOINED = ("src_img_path", "ref_img_path", "mask_path", "identity_file_path")


def test_get_args_has_the_reference_flags_and_defaults(golden):
    from face_mask_inpaint_amd.psp_inference import get_args

    ref = dict((k, v) for k, v in golden("psp_infer.pt")["args"])
    assert ref["output_size"] == 1024 and ref["batch_size"] == 8 and ref["use_attention"] == 0 and ref["use_ref"] is False  # the issue's list
    ours = vars(get_args([]))
    assert set(ref) <= set(ours), sorted(set(ref) - set(ours))
    for k, v in ref.items():
        if k not in PATH_ARGS:
            assert ours[k] == v and type(ours[k]) is type(v), (k, ours[k], v)
    for k in JOINED:  # the reference's value is os.path.join(data_root, <its default>): the sub-path default itself is kept
        assert ref[k] == os.path.join(ref["data_root"], ours[k]), k
    for k in ("data_root", "mask_detector_path", "pt_ckpt_path", "out_dir"):
        assert ours[k] is None, k  # nothing points outside the working directory
    assert ours["decoder_dtype"] == "fp32" and get_args(["--decoder_dtype", "bf16"]).decoder_dtype == "bf16"
    assert get_args(["--use_ref", "--save_src_mask", "1"]).use_ref is True


def test_host_tensor2im_equals_the_reference(golden):
    from face_mask_inpaint_amd.psp_inference import tensor2im, tensor2im_unit

    f = golden("psp_infer.pt")["tensor2im"]
    t = f["input"]
    assert t.shape == (3, 64, 64) and float(t.min()) < -1 and float(t.max()) > 1 and bool((t == 1).any()) and bool((t == -1).any())
    before = t.clone()
    got = np.array(tensor2im(t))
    assert got.dtype == np.uint8 and np.array_equal(got, f["psp_inference"].numpy())
    got = tensor2im_unit(t)
    assert got.dtype == np.uint8 and np.array_equal(got, f["gradio_serve"].numpy())
    assert torch.equal(t, before)  # neither writes into its argument
    assert len(np.unique(f["psp_inference"].numpy())) == 256  # the fixture walks through every output value


def test_image_tail_entries_are_declared():
    hdr = open(os.path.join(ROOT, "include", "fmi_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from face_mask_inpaint_amd import _lib

    for name in ("fmi_image_tail_f32", "fmi_planes_to_u8_f32"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES


def test_image_tail_argument_validation_without_a_gpu():
    """bad arguments come back as status codes before anything is launched (as test_c_abi_argument_validation_without_a_gpu)"""
    from face_mask_inpaint_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfmi_hip.so not built")
    c = ctypes.CDLL(_lib.LIB_PATH)
    BAD, UNSUP = 1, 2
    i32, f32, vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    c.fmi_image_tail_f32.argtypes = [vp, vp, vp, vp, i32, i32, f32, f32, vp]
    c.fmi_planes_to_u8_f32.argtypes = [vp, vp, i32, i32, i32, i32, f32, f32, vp]
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, vp)
    p = vp((p.value + 15) & ~15)  # 16-byte aligned inside the buffer
    assert c.fmi_image_tail_f32(None, p, p, p, 1, 256, 1.0, 0.5, None) == BAD            # x = NULL
    assert c.fmi_image_tail_f32(p, None, None, None, 1, 256, 1.0, 0.5, None) == BAD      # no output wanted
    assert c.fmi_image_tail_f32(p, p, None, None, 0, 256, 1.0, 0.5, None) == BAD         # N = 0
    assert c.fmi_image_tail_f32(p, p, None, None, -1, 1024, 1.0, 0.5, None) == BAD
    assert c.fmi_image_tail_f32(p, p, None, None, 1, 384, 1.0, 0.5, None) == UNSUP       # S outside 256 {1, 2, 4}
    assert c.fmi_image_tail_f32(p, None, None, p, 1, 128, 1.0, 0.5, None) == UNSUP
    assert c.fmi_image_tail_f32(p, vp(p.value + 4), None, None, 1, 256, 1.0, 0.5, None) == BAD   # misaligned output
    assert c.fmi_planes_to_u8_f32(None, p, 1, 1, 4, 4, 0.0, 1.0, None) == BAD
    assert c.fmi_planes_to_u8_f32(p, None, 1, 1, 4, 4, 0.0, 1.0, None) == BAD
    assert c.fmi_planes_to_u8_f32(p, p, 0, 1, 4, 4, 0.0, 1.0, None) == BAD
    assert c.fmi_planes_to_u8_f32(p, p, 1, 3, 0, 4, 0.0, 1.0, None) == BAD
    assert c.fmi_planes_to_u8_f32(p, p, 1, 2, 4, 4, 0.0, 1.0, None) == UNSUP             # one plane (replicated) or three


def test_harness_refuses_to_run_without_a_gpu(monkeypatch):
    from face_mask_inpaint_amd import psp_inference as PI
    from face_mask_inpaint_amd._lib import FmiError

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(FmiError):
        PI.main(["--num_batches", "1", "--batch_size", "1"])
    with pytest.raises(FmiError):
        PI.ModelInterface(PI.get_args([]))
    with pytest.raises(FmiError):
        from face_mask_inpaint_amd import functional as FF

        FF.image_tail(torch.zeros(1, 256, 256, 3))  # CPU tensor: refused, not computed


def test_fixture_files_respect_the_size_limit(golden):
    fx = golden("psp_infer.pt")
    names = ["psp_infer.pt"] + [os.path.join("psp_infer_parts", n + ".pt") for n in fx["parts"]]
    for n in names:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", n)) <= 1 << 20, n
    assert fx["config"]["output_size"] == 1024 and fx["att0"]["latent"].shape == (1, 18, 512)
