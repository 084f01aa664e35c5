"""How much of a k_trace4 launch lies behind the end of its work list (dev tool; needs a -DGX_TAIL_STAMP build):
GNXR_LIB=ab_libs/lib_stamp.so python tests/dev_tail_stamp.py [cfg3|cfg4|box]
Renders two steps of the headline run (1920 x 1080, 128 spp each; the first one is warm-up) and prints one JSON line: the device's 100 MHz
clock at the first fetch that reaches the stamped point and at the exit of the last wave, summed over the launches of the second step.
"box": the all-emissive slab of tests/test_nee_work_items.py instead (most vertices have a shadow ray AND a MIS ray).  With a library that has no
stamps (any build) the line holds the render and trace times only."""
import os, sys, json, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import gnxraytracer_amd as gx, scenes
workload = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
gx.init(0)
if workload == "box":
    import test_nee_work_items
    b = test_nee_work_items.emissive_box(gx)
else:
    b = scenes.dragon_cornell(100000, "glass+metal") if workload == "cfg3" else scenes.dragon_cornell(100000, "zoo", env=scenes.synthetic_env_path(1000, 500))
scene = gx.Scene(b); integ = gx.PathIntegrator(8, 1.0, "spatial")
out = torch.zeros((1080, 1920, 4), device="cuda")
lib = C.CDLL(gx.LIB_PATH)
buf = (C.c_ulonglong * 12)()
stamps = hasattr(lib, "gnxr_debug_tail_stamp")
gx.lib().gnxr_set_profiling(1)   # per-kernel timing: seconds_closest
integ.RenderDevice(scene, out.data_ptr(), 1920, 1080, 1024, spp_begin=0, spp_end=128)
torch.cuda.synchronize()
assert not stamps or lib.gnxr_debug_tail_stamp(buf, 1) == 0
st = integ.RenderDevice(scene, out.data_ptr(), 1920, 1080, 1024, spp_begin=128, spp_end=256)
torch.cuda.synchronize()
assert not stamps or lib.gnxr_debug_tail_stamp(buf, 1) == 0
v = list(buf)
ms = lambda t: round(t / 1e5, 3)   # 100 MHz ticks
d = {"lib": os.path.basename(gx.LIB_PATH), "workload": workload, "seconds_render": round(st["seconds_render"], 5), "seconds_trace": round(st["seconds_closest"], 5), "mis_rays": st["rays_closest_nee"], "shadow_rays": st["rays_any"], "rays": st["rays_closest"] + st["rays_any"],
     "all_launches": {"launches": v[6], "items": v[7], "kernel_ms": ms(v[5]), "behind_ms": ms(v[4]), "behind_frac": round(v[4] / max(1, v[5]), 4)},
     "launches_of_2^24_items_and_more": {"launches": v[10], "items": v[11], "kernel_ms": ms(v[9]), "behind_ms": ms(v[8]), "behind_frac": round(v[8] / max(1, v[9]), 4),
                                         "behind_ms_per_launch": ms(v[8] / max(1, v[10]))}}
if not stamps: d = {k: v for k, v in d.items() if not isinstance(v, dict)}
print(json.dumps(d))
