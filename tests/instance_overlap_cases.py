"""The set and boxes of the instanced box-overlap tests (tests/test_gpu_instance_overlap.py), made without a device so that what
they cover can be checked on the restatement alone (tests/test_instance_overlap_reference.py).

The set is instance_near_cases.nine_instances: seven placed copies of lobed_528 (instance 4 an exact duplicate of instance 1)
and the two tiny scenes.  The boxes are overlap_cases.make_boxes on the merged scene (the mapped corners in instance order):
voxel cells, boxes about surface points sized for a few, for more than 8 and for more than 64 triangles, zero-extent boxes,
boxes with a face on a vertex coordinate, far boxes and boxes that are not walked.  assert_mixed states what they must cover."""
from __future__ import annotations

import numpy as np

import instance_near_cases as NC
import instance_point_ref as IP
import overlap_cases as OC
import overlap_ref as OR

F = np.float32
NINE_BOXES, NINE_BOX_SEED = 1536, 21
FLOOR = 0.04

nine_instances = NC.nine_instances


def world_boxes(scene_positions, scene_of_instance, maps, n=NINE_BOXES, seed=NINE_BOX_SEED):
    """BOX_DTYPE world boxes of every kind of overlap_cases, over the merged scene"""
    merged, _ = IP.merged_positions(scene_positions, scene_of_instance, maps)
    return OC.make_boxes({"vertex_positions": merged}, n, seed)


def shares(boxes, instances64, counts) -> dict:
    """what assert_mixed measures, on the restatement's K = 64 answer"""
    walked = OR.walked(boxes)
    spans = lambda held: np.array([len(set(row[row >= 0].tolist())) for row in held])
    return {"touching nothing, walked": float((walked & (counts == 0)).mean()),
            "n 1 to 8": float(((counts >= 1) & (counts <= 8)).mean()),
            "n 9 to 64": float(((counts >= 9) & (counts <= 64)).mean()),
            "n above 64": float((counts > 64).mean()),
            "first 8 of two or more instances": float((spans(instances64[:, :8]) >= 2).mean()),
            "first 64 of two or more instances": float((spans(instances64) >= 2).mean())}


def assert_mixed(boxes, instances64, counts, code, what):
    """over 4 % of the boxes in each band of n and with held pairs of two or more instances among the first 8 and the first 64;
    and every axis after the box's own is the first to separate at least one pair (`code`: overlap_ref.first_axis on the
    merged scene)"""
    assert instances64.shape[1] == 64
    s = shares(boxes, instances64, counts)
    low = {k: v for k, v in s.items() if v <= FLOOR}
    assert not low, f"{what}: at or under {FLOOR:.0%} of {len(boxes)} boxes: {low} (all: {s})"
    per_axis = np.bincount(code[(code >= 0) & (code < OR.AXES)].astype(np.int64), minlength=OR.AXES)
    assert min(per_axis[3:]) >= 1, (what, per_axis.tolist())
    s["first to separate, per axis"] = per_axis.tolist()
    return s
