"""tests/golden/conv_plans.json: plans of the conv op recorded on an MI355X from the commit before the planner moved into
csrc/conv_plan.h.  "plans": each distinct outcome once, as tools/conv_plan_check prints it with the `key=` of every field
but the kernel's name left out (the keys, in the tool's order, are below), or "rc=<code> <message>" for a refusal.
"cases": [name, the 25 descriptor integers, the KEY=VALUE switches, the workgroups per CU the runtime answered, index
into "plans"].  dfx_conv_query, dfx_debug_conv_sched and dfx_debug_conv_unit_px reported fields of the plan itself at the
recording (checked when the file was written), so what they must report is derived here, not stored a second time."""
import json
import os

COMMON = "variant direct pw nw wo wo1 occ pxb icb ocb G grid block lds roles_ok rows_per_unit units_per_image".split()
RESIDENT = ["m." + k for k in ("th tw uy ux linear total_units row_chunks tile_chunks row_magic tw_magic upi_magic ux_magic ntu ntu_magic "
                               "claim_limit tile_stride static_rounds pool lazy_queue half_from upx").split()]
STREAM = ["s." + k for k in ("ni thv twv uy ux total_units lh lw npos n_icc icb n_occ ocb n_g1 ks2 s0_steps mid_stride off_tile off_pxoff "
                             "off_mid off_cst off_stage planes mg_g4 mg_lhw mg_lw occ_par").split()]
DIRECT = ["d." + k for k in ("ni thv twv uy ux total_units lh lw npos icb n_planes plane_bytes row_pitch img_pitch unfused ocb n_g1 "
                             "mid_stride off_pxoff off_mid off_cst npb").split()]
PW = ["p." + k for k in "icb ocb px_total n_blocks off_cst off_stage stage_bytes".split()]


def load():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans.json")) as f:
        g = json.load(f)
    g["cases"] = [dict(name=n, desc=[int(v) for v in d.split()], tuning=dict(kv.split("=", 1) for kv in t.split()), per_cu=w,
                       plan=g["plans"][i]) for n, d, t, w, i in g["cases"]]
    return g


def keys_of(values):
    """the field names of a plan's values, by the family its first three values name"""
    variant, direct, pw = int(values[0]), int(values[1]), int(values[2])
    fam = [] if variant == 0 else RESIDENT if variant in (1, 2) else STREAM if not direct else DIRECT + (PW if pw else [])
    return COMMON + fam


def fields(plan):
    """a golden plan (not a refusal) as {field: int} plus "name" """
    head, name = plan.split(" name=", 1)
    values = head.split(" ")
    keys = keys_of(values)
    assert len(keys) == len(values), plan
    p = {k: int(v) for k, v in zip(keys, values)}
    p["name"] = name
    return p


def hooks(p):
    """what the library's query hooks report for the plan `p` of fields(): (info fields, sched or None, unit_px)"""
    info = dict(variant=p["variant"], grid=p["grid"], block=p["block"], lds_bytes=p["lds"], rows_per_unit=p["rows_per_unit"],
                kernel_name=p["name"])
    if "m.th" not in p:
        return info, None, 0
    sched = [p["m." + k] for k in ("th", "tw", "linear", "uy", "ux", "total_units", "half_from", "static_rounds", "lazy_queue", "pool")]
    return info, sched + [2 * p["grid"], 0, 0], p["m.upx"]   # (teams; roles and ring waits are 0 before set_weights / submit)
