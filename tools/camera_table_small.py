"""The camera-vertex table on a SMALL render (Cornell 1080p, 1 or 2 frame slots, so one slot per jitter group, depth 1 or 2): with no
camera ray shared, is the table's round trip (32 B written and read per path) and its launch paid back by the two launches and the
extension-queue round trip that go away?  One context, the switch CAP_NO_CAMERA_TABLE flipped between blocks of renders, host clock
around a block that ends in a synchronise.  python tools/camera_table_small.py [slots] [depth] [renders per block] [rounds]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from capsaicin_amd import capi  # noqa: E402


def main():
    slots = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    depth = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    per = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w, h = 1920, 1080
    r = capi.Renderer(0)
    r.upload_geometry(capi.Geometry(os.path.join(root, "assets", "cornell_box.obj")))
    r.upload_bluenoise(capi.load_bluenoise())
    r.build_bvh()
    r.set_resolution(w, h)
    r.set_camera(capi.cornell_camera(w, h))
    frame = 0
    for off in (1, 0):  # warm-up: both forms' kernels loaded, the table allocated
        r.debug_switch("CAP_NO_CAMERA_TABLE", off)
        for _ in range(20):
            r.render(frame, slots, depth, 0)
            frame += slots
    r.sync()
    ms = {0: [], 1: []}
    for _ in range(rounds):
        for off in (1, 0):
            r.debug_switch("CAP_NO_CAMERA_TABLE", off)
            r.render(frame, slots, depth, 0)
            assert r.debug_get(r.DEBUG_CAMERA_TABLE) == 1 - off
            r.sync()
            t0 = time.perf_counter()
            for _ in range(per):
                r.render(frame, slots, depth, 0)  # frame_begin advances from call to call, as in real use
                frame += slots
            r.sync()
            ms[off].append((time.perf_counter() - t0) * 1e3 / per)
    for off in (1, 0):
        v = sorted(ms[off])
        print("slots %d depth %d  table %s  ms/render: median %.4f  min %.4f  max %.4f  (%s)" %
              (slots, depth, "off" if off else "on ", v[len(v) // 2], v[0], v[-1], " ".join("%.4f" % x for x in ms[off])))


if __name__ == "__main__":
    main()
