"""ltr_slate_metrics refuses bad arguments by return code before anything touches the device."""
import ctypes as C
import os

from vllm_ltr_amd import _lib


def test_slate_metrics_argument_errors_without_gpu():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    lib = _lib.load()
    assert lib.ltr_slate_metrics_workspace_bytes(2, 4097) == 0 and lib.ltr_slate_metrics_workspace_bytes((1 << 20) + 1, 8) == 0
    need = lib.ltr_slate_metrics_workspace_bytes(2, 65)
    assert need > 0

    def call(n_ats, S=65, y_pred=256, ws_bytes=need, ats=5, gain=0):       # (pointers are never followed: the checks come first)
        cfg = _lib.SlateMetricsConfig(n_ats, (C.c_int32 * 8)(*[ats] * 8), gain, -1.0, 1.0)
        return lib.ltr_slate_metrics(y_pred, 256, 2, S, C.byref(cfg), None, None, None, 256, 256, ws_bytes, None)
    for bad, word in (({"n_ats": 0}, b"n_ats"), ({"n_ats": 9}, b"n_ats"), ({"n_ats": 2, "S": 4097}, b"shape"),
                      ({"n_ats": 2, "y_pred": None}, b"NULL"), ({"n_ats": 2, "ats": 0}, b"cut-off"), ({"n_ats": 2, "gain": 2}, b"gain")):
        assert call(**bad) == _lib.LTR_E_INVAL == -22, bad
        assert word in lib.ltr_last_error(), (bad, lib.ltr_last_error())
    assert call(2, ws_bytes=need - 1) == _lib.LTR_E_NOMEM
    assert call(2, S=0) == 0                                               # an empty batch: nothing to do
