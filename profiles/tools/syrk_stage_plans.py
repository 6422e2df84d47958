"""Print sdpb_hip_memory_plan of the CPU-emulated library for the cases the tests use, one JSON line each (device.free_bytes
taken out), to compare two source trees: run it from the root of each tree after tests/emu/build_emu.py and diff the outputs.
(profiles/syrk_stage_isa.txt)"""
import hashlib
import json
import os
import random
import sys

sys.path.insert(0, os.getcwd())
from sdpb_amd.solver import SDPSolver          # noqa: E402
from sdpb_amd.synthetic import make_sdp        # noqa: E402
from tests import libs, parity                 # noqa: E402


def show(name, s):
    plan = s.memory_plan()
    plan["device"].pop("free_bytes", None)
    print(name, json.dumps(plan, sort_keys=True), flush=True)


sdp = make_sdp([1] * 6, [30] * 6, 150, 512, seed=13)
a = SDPSolver(sdp, 512, parity.DEFAULT_PARAMS, lib_path=libs.emu_lib())
show("synthetic_N150 default", a)
bound = a.memory_plan()["syrk"]["partial_bytes"] // 4
a.set_max_shared_memory(bound)
show("synthetic_N150 max_shared_memory=partial_bytes//4", a)
assert not a.iterate()
show("synthetic_N150 max_shared_memory=partial_bytes//4 after an iteration", a)
a.close()
sdp, meta, _, _ = parity.load_case("singlet_cT")
for bound in (0, 1_400_000, 3):
    s = SDPSolver(sdp, meta["precision"], meta["params"], lib_path=libs.emu_lib())
    if bound:
        s.set_max_shared_memory(bound)
    show(f"singlet_cT max_shared_memory={bound}", s)
    assert not s.iterate()
    show(f"singlet_cT max_shared_memory={bound} after an iteration", s)
    s.close()
sdp, meta, _, _ = parity.load_case("1d")
for precision, rows, cols, image, part in ((512, 140, 47, 6.0e5, 1.0e6), (1280, 70, 17, 8.0e4, 3.5e5)):
    os.environ.update(SDPB_HIP_SYRK_SPLITS="2", SDPB_HIP_SYRK_IMAGE_BYTES=str(int(image)), SDPB_HIP_SYRK_PART_BYTES=str(int(part)))
    s = SDPSolver(sdp, precision, lib_path=libs.emu_lib())
    fb = s.fx_frac_bits
    rng = random.Random(rows * 1000 + cols)
    vals = [rng.randrange(-(2 ** fb) + 1, 2 ** fb) for _ in range(rows * cols)]
    got = s.op_int_syrk(rows, cols, vals)
    show(f"1d {precision} bits after op_int_syrk({rows}, {cols}) SPLITS=2 IMAGE_BYTES={int(image)} PART_BYTES={int(part)}", s)
    print("   sha1 of the product:", hashlib.sha1(repr(got).encode()).hexdigest())
    s.close()
