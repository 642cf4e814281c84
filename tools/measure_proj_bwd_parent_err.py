"""PARENT_ERR of tests/test_gpu_fno_proj_bwd_fused.py: the float64 error of the PARENT commit's projection backward on the test's
cases.  Run on an MI355X against a checkout of the parent commit with its library built:

    python tools/measure_proj_bwd_parent_err.py /path/to/parent/checkout

The parent has no exported entry point for the projection backward with the MSE term, so its internal host routine
dlwp_pwmlp_bwd_rows_ex -- the one its rollout trainer calls; an ordinary C++ function of libdlwpmi.so -- is called through its
mangled name with the trainer's arguments (slab mode, pred / target, adjoint rows DFT).  The cases, tensors and the float64
reference are the test module's own; the block-0 launch in front is the parent's dlwp_fno_block_lift_bwd_slab.
"""
import ctypes as C
import importlib.util
import json
import os
import sys

ROWS_EX = ("_Z22dlwp_pwmlp_bwd_rows_exPK13dlwp_chan_srcPKfS3_S3_S1_S1_S1_fPK13dlwp_chan_dstiS6_PfS7_S7_S7_S7_iiiiii"
           "PK13dlwp_fno_planP15HIP_vector_typeIfLj2EEP12ihipStream_t")


def main():
    parent = os.path.abspath(sys.argv[1])
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, parent)
    import torch
    from dlwp_benchmark_amd import lib as L
    assert os.path.dirname(os.path.dirname(os.path.abspath(L.__file__))) == parent, L.__file__
    spec = importlib.util.spec_from_file_location("proj_bwd_cases", os.path.join(here, "..", "tests", "test_gpu_fno_proj_bwd_fused.py"))
    tc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tc)
    lib = L.load()
    V, I = C.c_void_p, C.c_int
    rows_ex = getattr(lib, ROWS_EX)
    rows_ex.restype = I
    rows_ex.argtypes = [V] * 7 + [C.c_float, V, I, V] + [V] * 5 + [I] * 6 + [V, V, V]
    dev = torch.device("cuda:0")
    res = {k: [] for k in tc.QUANT}
    for case in tc.CASES:
        B, Cc, Cin, Ch, PCh = case
        bench = tc.Bench(L, dev, case)
        d, P = bench.d, bench.P

        def proj(gy, gy_bstride, gcur, x1, slab_proj, acc):
            view = lambda ptr, bs: L.ChanSrc(ptr, bs, P, None, None)      # noqa: E731  (dlwp_chan_dst has the same layout)
            x, g, pr, tg = view(L.ptr(d["px"]), Cc * P), view(gy.data_ptr(), gy_bstride), view(L.ptr(d["pred"]), P), view(L.ptr(d["target"]), P)
            gx = view(L.ptr(gcur), Cc * P)
            L.check(rows_ex(C.byref(x), L.ptr(d["pw1"]), L.ptr(d["pb1"]), L.ptr(d["pw2"]), C.byref(g), C.byref(pr), C.byref(tg),
                            tc.MSE_SCALE, C.byref(gx), 0, None, None, None, None, None, L.ptr(slab_proj), acc, B, Cc, PCh, 1, P,
                            bench.plan, L.ptr(x1), L.stream()))

        out, _, gy_read = bench.run("two", proj)
        err = bench.errors(out, gy_read)
        bench.close()
        print(tc.case_id(case), err, flush=True)
        for k in tc.QUANT:
            res[k].append(err[k])
    print(json.dumps(res))
    for k in tc.QUANT:
        print('    "%s": [%s],' % (k, ", ".join("%.3e" % v for v in res[k])))


if __name__ == "__main__":
    main()
