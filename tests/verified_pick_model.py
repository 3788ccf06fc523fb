"""The verified pick of fl_recognize_batch_instances_verified (include/fealess_hip.h) as a plain loop, test infrastructure only.

A group's refined members come in list order.  found[r]: the member's fl_recognition_result::found; records: its finished
fl_verify_result (verify_model.DTYPE; all zero for a member that was not found); nms: the member nonMaximumSuppression's rule
picks (instances_model.pick); verified: the group's class passes class_idx.
"""
import numpy as np


def pick(found, records, nms, verified):
    """(picked member, the member whose record gets best = 1 or -1).  Python integers: the products are exact."""
    if not verified:
        return nms, -1
    best = -1
    for r in range(len(found)):
        if not found[r] or not int(records["accepted"][r]):
            continue
        if best < 0 or int(records["n_inlier"][r]) * int(records["n_model"][best]) > int(records["n_inlier"][best]) * int(records["n_model"][r]):
            best = r
    return (best if best >= 0 else nms), best


def nms_pick(found, n_points, dist_mean):
    """nonMaximumSuppression's choice among a group's refined members (the header's statement of it), 0 when none was found."""
    o, size_th = -1, 0
    for r in range(len(found)):
        if not found[r]:
            continue
        if o < 0:
            o, size_th = r, int(float(np.float32(n_points[r])) * 0.85)
        elif n_points[r] > size_th and dist_mean[r] < dist_mean[o]:
            o = r
    return max(o, 0)
