#!/usr/bin/env python
"""Host time per rtod_forward call of several BUILDS of librtod in ONE process (private dlopen per library, as tools/exp_ab_libs.py
does): CALLS back-to-back rtod_forward calls between two host clock reads with no synchronise inside the window (what the host pays
to enqueue the launch list), and the same window closed by a device synchronise (time to completion); interleaved rounds, the order
alternating, medians.  Each library autotunes its own tiles.
    python tools/exp_forward_host_cost.py NET res batch OPTS libA.so libB.so ...     (names relative to realtimeobjectdetection_amd/)
NET = yolov3 | yolov3-tiny; OPTS = name=value,... plan options ("" for none).  Environment: ROUNDS (40), CALLS (50)."""
import ctypes as C, os, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import numpy as np, torch
from realtimeobjectdetection_amd import cfgs, synth, _ffi
from realtimeobjectdetection_amd.cfg import parse_cfg_text, build_ir
from realtimeobjectdetection_amd.darknet import Darknet
NET = sys.argv[1]; res = int(sys.argv[2]); B = int(sys.argv[3])
OPTS = {k: int(v) for k, v in (kv.split("=") for kv in sys.argv[4].split(",") if kv)}
names = sys.argv[5:]
ROUNDS = int(os.environ.get("ROUNDS", "40")); CALLS = int(os.environ.get("CALLS", "50"))
here = os.path.dirname(os.path.abspath(_ffi.__file__))
handles = {}
for n in names:
    _ffi.LIB_PATH = os.path.join(here, n); _ffi._lib = None
    handles[n] = _ffi.lib()
def use(n): _ffi._lib = handles[n]
text = {"yolov3": cfgs.yolov3_cfg, "yolov3-tiny": cfgs.yolov3_tiny_cfg}[NET](); ir = build_ir(parse_cfg_text(text), res)
w = synth.synth_weights(ir)
x = torch.from_numpy(synth.synth_frames(B, res)).cuda()
d = tempfile.mkdtemp()
models = {}; outs = {}; ref = None
for n in names:
    use(n)
    m = Darknet(cfgs.write_cfg(os.path.join(d, "m.cfg"), text), True).eval()
    m.net_info["height"] = res; m.precision = "f16s3"; m.overflow_check = "off"
    m.options.update(OPTS)
    m.load_weight_stream(w)
    with torch.no_grad():
        m(x); y = m(x)
    torch.cuda.synchronize()
    if ref is None: ref = y.clone()
    elif not torch.equal(y, ref): print("!! output of", n, "differs from", names[0], "max abs", float((y - ref).abs().max()))
    models[n] = m; outs[n] = torch.empty_like(y)
print("launches:", models[names[0]]._info.n_launches, flush=True)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
xp = C.c_void_p(x.data_ptr())
host = {n: [] for n in names}; wall = {n: [] for n in names}
for r in range(ROUNDS + 2):
    order = names if r % 2 == 0 else names[::-1]
    for n in order:
        lib = handles[n]; plan = models[n]._plan; op = C.c_void_p(outs[n].data_ptr()); fwd = lib.rtod_forward
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            rc = fwd(plan, xp, B, op, stream)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert rc == 0
        if r >= 2:                                       # two warm-up rounds
            host[n].append((t1 - t0) / CALLS * 1e6); wall[n].append((t2 - t0) / CALLS * 1e6)
def med(v):
    v = np.asarray(v); m = float(np.median(v))
    return m, float(1.4826 * np.median(np.abs(v - m)) * 1.2533 / np.sqrt(len(v)))
print("%-22s %26s %26s   (us per rtod_forward call, median +- its standard error over %d interleaved rounds of %d calls)" % ("", "host (enqueue)", "to completion", ROUNDS, CALLS))
for n in names:
    print("%-22s %17.2f +- %.2f %17.2f +- %.2f  host %+6.2f%% vs %s" % ((n,) + med(host[n]) + med(wall[n]) + ((med(host[n])[0] / med(host[names[0]])[0] - 1) * 100, names[0])))
