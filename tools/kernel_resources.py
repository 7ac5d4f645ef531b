#!/usr/bin/env python3
"""Per-kernel resource table of the shipped gfx950 code objects.

Reads the AMDGPU metadata note (`llvm-readelf --notes`) of every code object bundled in
open_spiel_amd/libosg_hip.so and prints, for every `__global__` entry point: vector / accumulator / scalar
registers, spilled registers, scratch bytes per lane, static LDS, the launch bound the kernel was compiled for and
the wavefronts per SIMD the register count allows (gfx950: 512 VGPRs per SIMD lane in granules of 8, at most 8
wavefronts per SIMD).  Needs no GPU.

  python tools/kernel_resources.py                     # table on stdout
  python tools/kernel_resources.py --out profiles/r05_kernel_resources.txt
  python tools/kernel_resources.py --check             # exit 1 if a kernel named in HOT spills

`tools/gpu_validation.sh` runs it with --check so a spill in a hot kernel cannot come back unnoticed.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"

# Every kernel the bench line names (headline, legs and secondary workloads), plus the evaluator / judge kernels of the
# same configs (prefix match on the short name below): each either spills nothing and uses no scratch, or stands in
# KNOWN with the measurement that justified keeping it as it is.
HOT = [
    "k_step_c4std2", "k_step_c4std<", "k_step_hexvec<3, 2",
    "k_cfr_small<true, true, 3, 2, 2, false>", "k_cfr_split<3, false, 512, 3, false>", "k_cfr_split<3, false, 512, 0, false>", "k_cfr_split<3, true, 512, 0, false>",
    # their Discounted CFR instantiations (the last template argument)
    "k_cfr_small<true, true, 3, 2, 2, true>", "k_cfr_split<3, false, 512, 3, true>", "k_cfr_split<3, false, 512, 0, true>", "k_cfr_sub<8, false, true>",
    "k_env_step_x2<osg::C4T<6, 7, 4, unsigned long> >",
    "k_env_step<osg::C4T<6, 7, 4, unsigned long> >",
    "k_env_step_compact_x2<osg::C4T<6, 7, 4, unsigned long> >",
    "k_random_steps<osg::C4T<6, 7, 4, unsigned long> >",
    "k_cfr_sub<8, false, false>", "k_cfr_sub<8, true, false>", "k_mccfr_resident_flat<3>", "k_mcts_advance<osg::Ttt, true, true>", "k_mcts_wave<osg::HexT<3>, true, true, false>",
    "k_rollout<osg::HexT<3> >", "k_eval_jobs", "k_geval_", "k_policy_eval", "k_oneshot_allreduce<double>",
    "k_observation_rows<osg::C4T<6, 7, 4, unsigned long>", "k_fold_deltas",
    # the alpha-beta search of the probe's three workloads (tools/probe_minimax.py)
    "k_alpha_beta<osg::Ttt>", "k_alpha_beta<osg::C4T<6, 7, 4, unsigned long> >", "k_alpha_beta<osg::HexT<3> >",
]
# Hot kernels whose parked registers / scratch are known, measured and kept (the note says where the decision is recorded).
KNOWN = {
    "k_mcts_wave<osg::HexT<3>, true, true, false>":
        "26 scalar registers parked in vector lanes (v_readlane, no memory) at 7 waves per SIMD (44 up to round 5), no scratch "
        "since round 6's templated position (1.105e9 -> 1.13e9 simulations/s against the previous object, profiles/r06zq_*); the form without "
        "the parked registers measured 2.7 % slower (profiles/r05_ab_register_work.txt, osg_mcts_wave.hip above wave_search)",
    "k_geval_persist":
        "opt-in cross-check form of the large-tree evaluation (OSG_EVAL_PERSIST=1; the default is a launch per level, which "
        "measured faster: profiles/r06u_*): 16 scalar registers parked in vector lanes, no scratch",
    "k_cfr_sub<8, false, true>":
        "the Discounted CFR form of the same kernel: the code of k_cfr_sub<8, false, false> with the iteration's three factors in "
        "vector registers, a multiply per policy term and a select and a multiply per folded regret; same registers, same reasons",
    "k_cfr_sub<8, true, false>":
        "the CFR-BR pass set of the same kernel (round 6): the code of k_cfr_sub<8, false, false> with the effective-policy rows staged "
        "every pass; same registers, same reasons",
    "k_cfr_sub<8, false, false>":
        "the bin's 24 history descriptors stay in registers across the passes of a launch (round 6): that pushes 52 vector "
        "registers into scratch around the fold and still measured 9 730 -> 10 240 iterations/s against fetching them every "
        "pass with no scratch (profiles/r06p_*); ~180 scalar registers (the kernel's ~40 argument pointers) are parked in "
        "vector lanes: a v_readlane each (693 of the kernel's 5 500 instructions, no memory) — fetching them with s_load "
        "at their uses would put a scalar-cache round trip on the phases' dependent chains instead",
    "k_mccfr_resident_flat<3>":
        "976 B of scratch per lane BY DESIGN: the traverser's frames below the top two (40 B x 24 levels) have no room in "
        "LDS (tables 67 KB x 2 workgroups per CU) — two frames in registers measured -3.3 % (profiles/r05_ab_solvers.txt); no register spills",
    "k_mcts_advance<osg::Ttt, true, true>":
        "the one-root search: ONE searching wavefront per launch by construction (1 wave per SIMD is its occupancy whatever "
        "the register count), 72 scalar registers parked in vector lanes; round 6 took its node accesses off volatile "
        "(12.39 -> 11.68 ms per 1000-simulation search, profiles/r06d_one_root_noderef_ab.txt)",
    "k_alpha_beta<osg::HexT<3> >":
        "36 scalar registers parked in vector lanes (v_readlane, no memory), no scratch, no LDS, 5 waves per SIMD: the hex(9) "
        "parameter block (five 3-word bit sets) beside a frame of 12 eight-byte words in registers — no form without them has been measured",
    "k_rollout<osg::HexT<3> >":
        "41 scalar registers parked in vector lanes (v_readlane, no memory), no scratch, 6 waves per SIMD; RandomRolloutEvaluator "
        "of hex(9) outside the search kernel (config 4's playouts run inside k_mcts_wave) — no form without them has been measured",
}


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return p.stdout.split("\n")[:len(names)]


def code_objects(lib, tmp):
    """Unbundle every gfx950 code object of `lib` into tmp; returns their paths."""
    dst = os.path.join(tmp, os.path.basename(lib))
    shutil.copy(lib, dst)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", dst], capture_output=True, text=True, check=True)
    return sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if "amdgcn" in f)


def kernels_of(obj):
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], capture_output=True, text=True, check=True).stdout
    m = re.search(r"^\s*---\n(.*?)^\s*\.\.\.\s*$", txt, re.S | re.M)
    if not m:
        return []
    # the note is indented by the tool only on its first lines; the YAML document itself starts at column 0
    meta = yaml.safe_load(m.group(1))
    return meta.get("amdhsa.kernels", [])


def waves_per_simd(vgpr, agpr):
    tot = vgpr + agpr
    if tot <= 0:
        return 8
    gran = (tot + 7) // 8 * 8
    return max(1, min(8, 512 // gran))


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"\(.*\)$", "", name)           # drop the parameter list
    name = name.replace("void ", "")
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "open_spiel_amd", "libosg_hip.so"))
    ap.add_argument("--out")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()

    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for obj in code_objects(a.lib, tmp):
            ks = kernels_of(obj)
            names = demangle([k[".name"] for k in ks])
            for k, n in zip(ks, names):
                rows.append(dict(
                    name=short(n), full=n,
                    vgpr=k.get(".vgpr_count", 0), agpr=k.get(".agpr_count", 0), sgpr=k.get(".sgpr_count", 0),
                    vspill=k.get(".vgpr_spill_count", 0), sspill=k.get(".sgpr_spill_count", 0),
                    scratch=k.get(".private_segment_fixed_size", 0), lds=k.get(".group_segment_fixed_size", 0),
                    bound=k.get(".max_flat_workgroup_size", 0), dyn=k.get(".uses_dynamic_stack", False)))
    rows.sort(key=lambda r: r["name"])

    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    lines = [
        f"# kernel resources of {os.path.relpath(a.lib, ROOT)} (gfx950), tree at {head}; tools/kernel_resources.py",
        "# vgpr/agpr/sgpr = registers allocated; vsp/ssp = registers spilled; scr = scratch bytes per lane; lds = static LDS bytes",
        "# (dynamic LDS is asked for at launch and not shown); wg = launch bound; w/simd = wavefronts per SIMD the VGPR count allows",
        f"# {len(rows)} entry points",
        f"{'vgpr':>4} {'agpr':>4} {'sgpr':>4} {'vsp':>4} {'ssp':>4} {'scr':>5} {'lds':>6} {'wg':>5} {'w/simd':>6}  kernel",
    ]
    bad = []
    for r in rows:
        flag = ""
        if r["vspill"] or r["sspill"] or r["scratch"]:
            flag = "  <-- spills" if (r["vspill"] or r["sspill"]) else "  <-- scratch (frames / dynamic indexing)"
        lines.append(f"{r['vgpr']:>4} {r['agpr']:>4} {r['sgpr']:>4} {r['vspill']:>4} {r['sspill']:>4} {r['scratch']:>5} "
                     f"{r['lds']:>6} {r['bound']:>5} {waves_per_simd(r['vgpr'], r['agpr']):>6}  {r['name']}{flag}")
        if any(r["name"].startswith(h) for h in HOT) and (r["vspill"] or r["sspill"] or r["scratch"]) and r["name"] not in KNOWN:
            bad.append(r["name"])
    n_spill = sum(1 for r in rows if r["vspill"] or r["sspill"])
    n_scr = sum(1 for r in rows if r["scratch"])
    lines.append(f"# {n_spill} of {len(rows)} entry points spill registers; {n_scr} use scratch")
    if bad:
        lines.append("# HOT kernels that spill: " + "; ".join(bad))
    else:
        lines.append("# every kernel of the HOT list (tools/kernel_resources.py) either spills nothing and uses no scratch or is listed under `known` below")
    for r in rows:
        if r["name"] in KNOWN:
            lines.append(f"# known: {r['name']}: {r['sspill']} scalar / {r['vspill']} vector registers spilled, {r['scratch']} B scratch — {KNOWN[r['name']]}")
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    if a.check and bad:
        sys.stderr.write("hot kernels spill: " + "; ".join(bad) + "\n")
        sys.exit(1)


if __name__ == "__main__":
    main()
