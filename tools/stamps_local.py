"""Where the wavefronts of one k_pass_chunks launch spend their time, by how much they evaluated (measurement build only).

Build a library with -DTSC_DBG_STAMPS (tools/build_variant.py NAME -DTSC_DBG_STAMPS) and run
    TSCODE_AMD_LIB=$PWD/tscode_amd/ab_libs/NAME.so python tools/stamps_local.py C3 1000 500 200 [opt=value ...]
The kernel stamps the 100 MHz wall clock at 0 wavefront started, 1 chunk ranked and stop columns found, 2 first evaluation stage entered,
4 last evaluation stage left, 3 the wavefront's tiles done, 5 rows applied; slot 6 holds sign batches + 65536 * exact batches
(local_pass.hpp).  Printed per pass: median and maximum of every segment over the wavefronts of each class -- no batch, one sign batch,
more than one -- and the segments of the wavefront that stamped the launch's last 5 (a launch is as long as its slowest wavefront).
"""
import ctypes as C
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from tscode_amd.pipeline import DevicePipeline
from tscode_amd.synthetic import make_config

cfg = sys.argv[1]
ks = [int(x) for x in sys.argv[2:] if "=" not in x]
pipe = DevicePipeline(make_config(cfg), 0)
for opt in sys.argv[2:]:
    if "=" in opt:
        pipe.set_option(opt.split("=")[0], float(opt.split("=")[1]))
for _ in range(3):
    pipe.step()
lib, h = pipe.engine.lib, pipe.engine._h
lib.tsc_debug_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
cap = 1 << 20
buf = np.zeros((cap, 8), dtype=np.uint64)


def us(x):
    return f"{np.median(x) / 100.0:6.2f} {x.max() / 100.0:6.2f}" if len(x) else "     -      -"


for k in ks:
    pipe.set_option("dbg_stamp_k", k)
    pipe.step()
    torch.cuda.synchronize()
    n = C.c_int64()
    assert lib.tsc_debug_stamps(h, buf.ctypes.data, cap, C.byref(n)) == 0
    s = buf[: n.value].astype(np.int64)
    s = s[s[:, 0] > 0]
    t0 = s[:, 0].min()
    sign, exact = s[:, 6] & 0xFFFF, s[:, 6] >> 16
    ranked = s[:, 1] > 0
    print(f"{cfg} k = {k}: {n.value} wavefronts, {len(s)} started, {int(ranked.sum())} in an open pass; first start -> last stamp "
          f"{(s[:, :6].max() - t0) / 100.0:.2f} us; sign batches {int(sign.sum())}, exact batches {int(exact.sum())}")
    print("class              wavefronts | 0->1 med max | 1->2 med max | 2->4 med max | 4->5 med max | 1->5 med max | 5 after first start: med max")
    for name, m in (("no batch", ranked & (s[:, 2] == 0)), ("one sign batch", ranked & (sign == 1)), ("more than one", ranked & (sign > 1)),
                    ("sign 0, exact > 0", ranked & (sign == 0) & (s[:, 2] > 0))):
        w = s[m]
        if not len(w):
            continue
        ev = w[:, 2] > 0
        print(f"{name:18s} {len(w):10d} | {us(w[:, 1] - w[:, 0])} | {us(w[ev, 2] - w[ev, 1])} | {us(w[ev, 4] - w[ev, 2])} | {us(w[ev, 5] - w[ev, 4])} | "
              f"{us(w[:, 5] - w[:, 1])} | {us(w[:, 5] - t0)}")
    last = s[np.argmax(s[:, 5])]
    seg = [f"start +{(last[0] - t0) / 100.0:.2f}", f"0->1 {(last[1] - last[0]) / 100.0:.2f}"]
    if last[2] > 0:
        seg += [f"1->2 {(last[2] - last[1]) / 100.0:.2f}", f"2->4 {(last[4] - last[2]) / 100.0:.2f}", f"4->5 {(last[5] - last[4]) / 100.0:.2f}"]
    else:
        seg += [f"1->5 {(last[5] - last[1]) / 100.0:.2f}"]
    print(f"the wavefront that ends the launch: {', '.join(seg)} us; sign batches {int(last[6] & 0xFFFF)}, exact batches {int(last[6] >> 16)}")
pipe.set_option("dbg_stamp_k", -1)
