"""The sample table on a SMALL render (Cornell 1080p, 1 frame slot, depth 1, no feedback): is the one extra launch per batch, k_sample_terms,
paid back by bounce 0's kernel?  One context, the switch CAP_SAMPLE_TABLE flipped between blocks of renders, host clock around a block
that ends in a synchronise.  python tools/sample_table_small.py [renders per block] [rounds] [depth]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from capsaicin_amd import capi  # noqa: E402


def main():
    per = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    depth = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w, h = 1920, 1080
    r = capi.Renderer(0)
    r.upload_geometry(capi.Geometry(os.path.join(root, "assets", "cornell_box.obj")))
    r.upload_bluenoise(capi.load_bluenoise())
    r.build_bvh()
    r.set_resolution(w, h)
    r.set_camera(capi.cornell_camera(w, h))
    frame = 0
    for on in (0, 1):  # warm-up: both forms' kernels loaded, the table allocated
        r.debug_switch("CAP_SAMPLE_TABLE", on)
        for _ in range(20):
            r.render(frame, 1, depth, 0)
            frame += 1
    r.sync()
    ms = {0: [], 1: []}
    for _ in range(rounds):
        for on in (0, 1):
            r.debug_switch("CAP_SAMPLE_TABLE", on)
            r.render(frame, 1, depth, 0)
            assert r.debug_get(r.DEBUG_SAMPLE_TABLE) == on
            r.sync()
            t0 = time.perf_counter()
            for _ in range(per):
                r.render(frame, 1, depth, 0)  # frame_begin advances from call to call, as in real use
                frame += 1
            r.sync()
            ms[on].append((time.perf_counter() - t0) * 1e3 / per)
    for on in (0, 1):
        v = sorted(ms[on])
        print("table %s  ms/render: median %.4f  min %.4f  max %.4f  (%s)" % ("on " if on else "off", v[len(v) // 2], v[0], v[-1], " ".join("%.4f" % x for x in ms[on])))


if __name__ == "__main__":
    main()
