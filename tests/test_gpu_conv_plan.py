"""The conv op's planner as the library runs it (csrc/conv_plan.h behind dfx_conv_create) against
tests/golden/conv_plans.json (tests/conv_plan_golden.py), recorded on an MI355X from the commit before the planner left
dfx_api.hip: for every case the handle is created under the case's switches and dfx_conv_query, dfx_debug_conv_sched and
dfx_debug_conv_unit_px must report the recorded plan's fields; a refused case must be refused with the same code and the
same dfx_last_error text.  The golden's grid of a streamed / direct / pointwise op was derived from the workgroups per CU
the runtime answered at the recording: the library asks again here, so a changed answer shows as a grid mismatch.
Launches no kernel and allocates no tensor (the 4 GiB cases cost nothing); tests/test_conv_plan_cpu.py checks the same
golden, field by field, without a GPU."""
import ctypes
import importlib

import pytest

import conv_plan_golden as G


@pytest.mark.gpu
def test_created_handles_match_the_recorded_plans():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    capi = importlib.import_module("deep-fusion_amd.capi")
    lib = capi.lib()
    g = G.load()
    assert torch.cuda.get_device_properties(0).multi_processor_count == g["ncu"], "the golden was recorded on an MI355X"
    torch.cuda.set_device(0)
    fields = [n for n, _ in capi.ConvDesc._fields_]
    bad = []
    for c in g["cases"]:
        d = capi.ConvDesc()
        for n, v in zip(fields, c["desc"]):
            setattr(d, n, v)
        h = ctypes.c_void_p()
        try:
            for k, v in c["tuning"].items():
                capi.set_tuning(k, v)
            rc = lib.dfx_conv_create(ctypes.byref(d), ctypes.byref(h))
            if rc:
                got = "rc=%d %s" % (rc, lib.dfx_last_error().decode())
                want = c["plan"]
                assert not h.value
            elif c["plan"].startswith("rc="):
                got, want = "created", c["plan"]
            else:
                info = capi.ConvInfo()
                assert lib.dfx_conv_query(h, ctypes.byref(info)) == 0
                v = (ctypes.c_int32 * 13)()
                src = lib.dfx_debug_conv_sched(h, v, 13)
                got = (dict(variant=info.variant, grid=info.grid, block=info.block, lds_bytes=info.lds_bytes,
                            rows_per_unit=info.rows_per_unit, kernel_name=info.kernel_name.decode()),
                       list(v) if src == 0 else [src, lib.dfx_last_error().decode()], lib.dfx_debug_conv_unit_px(h))
                winfo, wsched, wupx = G.hooks(G.fields(c["plan"]))
                want = (winfo, wsched or [2, "conv_sched: this op has no unit queue (%s)" % winfo["kernel_name"]], wupx)
        finally:
            for k in c["tuning"]:
                capi.set_tuning(k, None)
            if h.value:
                assert lib.dfx_conv_destroy(h) == 0
        if got != want:
            bad.append((c["name"], got, want))
    assert not bad, "%d of %d cases differ from the recording, the first: %r" % (len(bad), len(g["cases"]), bad[0])
