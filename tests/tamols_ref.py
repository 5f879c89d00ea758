"""Loader of the recorded reference cases tests/golden/tamols_ref_*.npz (oracle/record_tamols_reference.py wrote
them; tests only).  The case list is spelled out so a missing fixture fails instead of shrinking the tests."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TAMOLS_REF_CASES = (
    "shape_1x1", "shape_1x7", "shape_13x1", "shape_3x5", "shape_13x7", "shape_16x16", "shape_16x20",
    "backward_aliengo", "slow_b2", "no_velocity", "no_base", "base_ahead", "foot_on_patch_point", "all_infeasible",
    "some_infeasible", "no_ground_nan", "stacked_primitives")


@functools.lru_cache(maxsize=None)
def tamols_ref_config():
    z = np.load(os.path.join(GOLDEN, "tamols_ref_config.npz"))
    return dict(tamols_params=json.loads(str(z["tamols_params_json"])), robot=str(z["robot"]),
                cases=[str(c) for c in z["cases"]])


@functools.lru_cache(maxsize=None)
def tamols_ref_case(name):
    """One recorded case: the scene, the inputs (None where the reference got None), the reference's outputs.  The
    arrays are shared between the tests: do not write to them."""
    z = np.load(os.path.join(GOLDEN, f"tamols_ref_{name}.npz"))
    prims = [dict(type=int(r[0]), cx=r[1], cy=r[2], cz=r[3], a=r[4], b=r[5], c=r[6], yaw=r[7])
             for r in z["prims"].tolist()]
    hfield = None
    if bool(z["has_hfield"]):
        x0, y0, dx, dy = z["hfield_geo"].tolist()
        hfield = dict(z=z["hfield_z"], x0=x0, y0=y0, dx=dx, dy=dy)
    c = dict(name=name, robot=str(z["robot"]), rows=int(z["rows"]), cols=int(z["cols"]),
             params=json.loads(str(z["params_json"])),
             scene=dict(prims=prims, has_ground=bool(z["has_ground"]), ground_z=float(z["ground_z"]), hfield=hfield,
                        miss_z=float(z["miss_z"])),
             yaw=float(z["yaw"]), dist_x=float(z["dist_x"]), dist_y=float(z["dist_y"]), ray_z=float(z["ray_z"]),
             patches=z["patches"], seeds=z["seeds"], hips=z["hips"],
             vel=z["vel"] if bool(z["has_vel"]) else None, base=z["base"] if bool(z["has_base"]) else None,
             contact=z["contact"] if bool(z["has_contact"]) else None, feet=z["feet"] if bool(z["has_feet"]) else None,
             scores=z["scores"], footholds=z["footholds"], boxes=z["boxes"], valid=z["valid"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c
