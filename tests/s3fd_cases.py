"""Inputs shared by the S3FD tests: the cases tests/golden/make_s3fd_golden.py recorded (the frames
are regenerated from their keys), the synthetic network, and the tolerances derived from the forward
bound."""
import functools

import numpy as np

from s2v_amd import synth

# (frame key, batch, H, W) of the fixture's cases (make_s3fd_golden.py CASES)
CASES = {"main": ("s3fd.main", 3, 137, 181), "small": ("s3fd.small", 2, 64, 64)}
FORWARD_RTOL = 1e-3        # per map: max|d| <= 1e-3 * max(1, max|ref|) (test_retinaface_forward_matches_oracle's bound)

SMOOTH_CASES = {
    "smooth3": [[10, 20, 110, 140], [13, 22, 108, 139], [17, 27, 115, 150]],
    "smooth5": [[40, 31, 90, 101], [43, 30, 97, 99], [41, 36, 92, 108], [47, 33, 99, 104], [52, 39, 101, 111]],
    "smooth9": [[5, 8, 61, 77], [9, 8, 64, 75], [6, 13, 70, 81], [12, 11, 66, 84], [15, 17, 73, 80], [11, 21, 77, 88],
                [19, 18, 75, 93], [22, 26, 82, 90], [18, 29, 86, 97]],
}
FD_HW = (90, 120)
FD_RECTS = [(30, 20, 80, 60), (33, 22, 85, 66), (0, 0, 70, 75), (36, 25, 119, 85), (41, 29, 90, 71), (38, 33, 93, 78)]
FD_PADS = (7, 12, 35, 9)


def frames(case):
    """uint8 [B,H,W,3] frames as FaceAlignment.get_detections_for_batch receives them; the detector
    itself sees them with the channel order reversed (api.py:65)."""
    key, n, h, w = CASES[case]
    return synth.sr_frame(key, n, h, w)


@functools.lru_cache(maxsize=None)
def state_dict():
    from s2v_amd.models.s3fd_arch import S3FDParams
    return synth.s3fd_state_dict(S3FDParams())


def level_first(g, case):
    """First position index of each level (and the total) from the fixture's map shapes."""
    sizes = [g[f"{case}_map{2 * lv}"].shape[2] * g[f"{case}_map{2 * lv}"].shape[3] for lv in range(6)]
    return np.concatenate([[0], np.cumsum(sizes)])


def level_eps(g, case):
    """Per level, the forward bound evaluated on the fixture's conf logits."""
    return np.array([FORWARD_RTOL * max(1.0, float(np.abs(g[f"{case}_map{2 * lv}"]).max())) for lv in range(6)])
