"""CPU-only: ltr_head_encoder_create validates its arguments without touching the device."""
import ctypes as C

from vllm_ltr_amd import _lib


def test_encoder_create_argument_errors_without_gpu():
    lib = _lib.load()
    desc = _lib.HeadDesc()
    desc.n_features, desc.n_fc, desc.d_output, desc.weight_dtype = 64, 0, 1, _lib.LTR_W_F16
    fake = (C.c_void_p * 4)(0, 0, 64, 64)          # never dereferenced: create stores the pointers
    head, enc = C.c_void_p(), C.c_void_p()
    assert lib.ltr_head_create(C.byref(desc), fake, 4, C.byref(head)) == 0
    ptrs = (C.c_void_p * 14)(*[64] * 14)
    ed = _lib.HeadEncoderDesc(1, 128, 4, 0)
    assert lib.ltr_head_encoder_create(head, C.byref(ed), ptrs, 14, C.byref(enc)) == 0
    assert lib.ltr_head_encoder_workspace_bytes(enc, 10) > 10 * (64 * 5 + 128) * 4
    assert lib.ltr_head_encoder_destroy(enc) == 0
    assert lib.ltr_head_encoder_create(head, C.byref(ed), None, 14, C.byref(enc)) == -22
    assert lib.ltr_head_encoder_create(None, C.byref(ed), ptrs, 14, C.byref(enc)) == -22
    ed.h = 5
    assert lib.ltr_head_encoder_create(head, C.byref(ed), ptrs, 14, C.byref(enc)) == -22
    assert b"does not divide" in lib.ltr_last_error()
    assert lib.ltr_head_destroy(head) == 0
