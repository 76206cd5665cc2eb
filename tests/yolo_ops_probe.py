"""Helper of tests/test_gpu_yolo_ops.py: runs every crafted conv case of tests/yolo_ops_util.py under whatever TSTAR_YOLO_*
policy the parent set (the library reads it once per process) and saves, per case, the destination buffer after the run and
the kernel form the launcher reported.

    python tests/yolo_ops_probe.py <out.npz>
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yolo_ops_util as OU  # noqa: E402
from tstar_amd.yolo import FORM_NAMES, YoloDetector  # noqa: E402

out = {}
for B in (1, 2, 3):
    cases = [c for c in OU.CONV_CASES if c.B == B]
    prog, where = OU.conv_program(cases)
    det = YoloDetector.from_program(prog, max_batch=OU.MAX_BATCH)
    data = [OU.conv_data(c) for c in cases]
    for c, d, w in zip(cases, data, where):
        det.write_buffer(w["dst"], torch.from_numpy(d.dst).cuda(), OU.MAX_BATCH)
        if not c.same_buf:
            det.write_buffer(w["src"], torch.from_numpy(d.src).cuda(), OU.MAX_BATCH)
        if c.mode == "gate":
            det.write_buffer(w["aux"], torch.from_numpy(d.aux).cuda(), OU.MAX_BATCH)
    forms = det.run_ops(B)
    for c, d, w in zip(cases, data, where):
        out["out/" + c.name] = det.read_buffer(w["dst"], OU.MAX_BATCH).cpu().numpy()
        out["form/" + c.name] = np.array(FORM_NAMES[int(forms[w["op"]])])
        if not c.same_buf:                                   # a conv never writes its source
            assert np.array_equal(det.read_buffer(w["src"], OU.MAX_BATCH).cpu().numpy().view(np.uint32), d.src.view(np.uint32)), c.name
    det.close()
np.savez(sys.argv[1], **out)
print("PROBE_OK", len(out) // 2)
