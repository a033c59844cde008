"""Builds libpm_hip.so (the C-ABI library of include/pm.h) for gfx950 with hipcc, in-tree.

    python -m points_matching_amd.build [--force] [--verbose]

One object per translation unit, then one shared library next to this file.  Flags that matter
for parity: -ffp-contract=off (the only fused multiply-adds are the explicit fma()/fmaf() calls
the spec names) and hipcc's default correctly-rounded fp32 divide/sqrt, which must stay on.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libpm_hip.so")
SOURCES = ["pm_capi.cpp", "knn_l2.hip", "knn_coarse.hip", "knn_hamming.hip", "ransac.hip", "ransac_fused.hip", "ransac_shard.hip", "filter_gather.hip",
           "ransac_h_fused.hip", "homography_refine.hip", "ransac_a_fused.hip", "affine_refine.hip",
           "essential_solve.hip", "ransac_e_fused.hip", "recover_pose.hip", "pnp_solve.hip", "ransac_p_fused.hip",
           "pnp_refine.hip", "fundamental_refine.hip", "pose_refine.hip", "estimators.cpp", "match_cross.cpp",
           "pair_batch.cpp", "lmeds.hip", "mgpu.cpp", "flann.hip", "knn_guided.hip", "match_guided.cpp", "features.hip", "track_lk.hip",
           "corners.hip", "describe_points.hip", "warp.hip", "undistort.hip", "stereo.hip", "stereo_sgm.hip", "triangulate.hip",
           "align3d_solve.hip", "ransac_align3d_fused.hip", "align3d_refine.hip", "vocab.hip", "bowdb.hip", "bundle_adjust.hip", "pose_graph.hip"]
# per-file extra flags: the coarse kernels only nominate candidates (no result bit depends on them)
EXTRA = {"knn_coarse.hip": ["-ffinite-math-only"], "mgpu.cpp": ["-pthread"],
         # one 512-thread workgroup holding 45 fp64 partial sums per thread: report its registers and spills
         "homography_refine.hip": ["-Rpass-analysis=kernel-resource-usage"],
         "affine_refine.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # lane-serial fp64 5-point solver (its 10 x 20 elimination matrix lives in scratch) and the one-workgroup pose
         # recovery: report their registers, scratch and spills
         "essential_solve.hip": ["-Rpass-analysis=kernel-resource-usage"],
         "recover_pose.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # lane-serial fp64 P3P solver and the PnP scorer with its 5-plane LDS tile
         "pnp_solve.hip": ["-Rpass-analysis=kernel-resource-usage"],
         "ransac_p_fused.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # one 512-thread workgroup holding 28 fp64 partial sums per thread (S40)
         "pnp_refine.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # one 512-thread workgroup each: 45 / 36 fp64 partial sums per thread (S44, S45) and 21 (S47)
         "fundamental_refine.hip": ["-Rpass-analysis=kernel-resource-usage"],
         "pose_refine.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # the compaction with its three predicates (ratio, midpoint, cross-check S41): none may use scratch
         "filter_gather.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # guided k-NN (S48-S49): one wave per query, per-lane key lists; no instantiation may spill
         "knn_guided.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # feature front end (S53-S57): the descriptor kernel keeps its records in LDS and must not spill
         "features.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # Lucas-Kanade tracking (S61-S66): one wave per point with three int16 planes in LDS; lk_track must not spill
         "track_lk.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # Shi-Tomasi corners (S67-S70): corner_extrema holds 60 KiB of LDS planes, corner_select 8 conflict words per thread;
         # neither may use scratch or spill
         "corners.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # point descriptors (S71-S74): one wave per point with its patch and two u16 planes in LDS; desc_points must not spill
         "describe_points.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # image warp and point transform (S75-S78): four pixels per thread with fp64 positions; warp_bilinear must not spill
         "warp.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # lens distortion (S79-S83): fp64 polynomial positions, four pixels per thread; no kernel may use scratch or spill
         "undistort.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # dense stereo (S84-S88): a lane owns a disparity, two image tiles and a ring of column sums in LDS; no kernel may use
         # scratch or spill
         "stereo.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # semi-global matching (S89-S92): a wave walks a path with a lane per disparity, the next step's words and sums loaded
         # ahead; no kernel may use scratch or spill
         "stereo_sgm.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # triangulation (S93-S96): a lane owns a point, its 2V x 4 fp64 system and V pixels in registers, one instantiation per
         # view count; none may use scratch or spill
         "triangulate.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # 3-D alignment (S97-S101): the lane-serial fp64 triad solve, the scorer with its 6-plane LDS tile and the one-workgroup
         # refit with its 4 x 4 Jacobi in registers; none may use scratch or spill
         "align3d_solve.hip": ["-Rpass-analysis=kernel-resource-usage"],
         "ransac_align3d_fused.hip": ["-Rpass-analysis=kernel-resource-usage"],
         "align3d_refine.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # visual vocabularies (S102-S106): the scatter-reduction keeps a run's sums in registers (8 counters per lane on 512-bit
         # rows); no kernel may use scratch or spill
         "vocab.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # image database (S107-S112): one wave per image with four entry loads in flight, and a 1024-thread selection with
         # its 2048 keys in LDS; no kernel may use scratch or spill
         "bowdb.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # local bundle adjustment (S113-S117): one 512-thread workgroup, at most 42 fp64 partial sums per thread and the
         # 42 x 42 reduced system in LDS; it must not use scratch or spill
         "bundle_adjust.hip": ["-Rpass-analysis=kernel-resource-usage"],
         # pose-graph optimisation (S118-S123): one 512-thread workgroup, a node's 28 + 7 fp64 sums per thread and the Jacobian
         # rows streamed from the workspace; it must not use scratch or spill
         "pose_graph.hip": ["-Rpass-analysis=kernel-resource-usage"]}
RESOURCE_LINES = ("Function Name", "VGPRs:", "ScratchSize", "Spill")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wall", "-Wno-unused-function",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I/opt/rocm/include"]


def _newer(a, b):
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def _deps():
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".h"))]
    hdrs.append(os.path.join(ROOT, "include", "pm.h"))
    hdrs.append(os.path.abspath(__file__))
    return hdrs


def build(force=False, verbose=False, extra_flags=()):
    os.makedirs(OBJ, exist_ok=True)
    deps = _deps()
    jobs = []
    objs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src.rsplit(".", 1)[0] + ".o")
        objs.append(o)
        if force or _newer(s, o) or any(_newer(d, o) for d in deps):
            cmd = [HIPCC] + FLAGS + EXTRA.get(src, []) + list(extra_flags) + (["-x", "hip"] if src.endswith(".hip") else []) + \
                  ["-c", s, "-o", o]
            jobs.append(cmd)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n%s\n%s" % (" ".join(cmd), r.stderr))
        if verbose and r.stderr.strip():
            print(r.stderr)
        elif "-Rpass-analysis=kernel-resource-usage" in cmd:
            for line in r.stderr.splitlines():
                if "remark:" in line and any(k in line for k in RESOURCE_LINES):
                    print(os.path.basename(cmd[cmd.index("-c") + 1]) + ": " +
                          line.split("remark:", 1)[1].replace("[-Rpass-analysis=kernel-resource-usage]", "").strip())

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if force or jobs or not os.path.exists(LIB):
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl", "-pthread"])
    return LIB


HOST_DIR = os.path.join(HERE, "host")
HOST_SRC = os.path.join(HOST_DIR, "pm_cli.cpp")
HOST_SRCS = [HOST_SRC, os.path.join(HOST_DIR, "pm_features.cpp")]
HOST_BIN = os.path.join(HOST_DIR, "pm_cli")


def build_host(force=False):
    """C++ host tool (the counterpart of the reference's main()); links libpm_hip.so."""
    if not os.path.exists(HOST_SRC):
        return None
    deps = HOST_SRCS + [os.path.join(HOST_DIR, "pm_features.hpp"), os.path.join(ROOT, "include", "pm.h"), LIB]
    if force or any(_newer(d, HOST_BIN) for d in deps):
        cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + HOST_DIR] + HOST_SRCS + \
              ["-o", HOST_BIN, "-L" + HERE, "-lpm_hip", "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath," + HERE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("host build failed:\n%s\n%s" % (" ".join(cmd), r.stderr))
    return HOST_BIN


def build_host_sanitized():
    """The host tool under AddressSanitizer + UBSan (tests/test_oracle_sanitized_cpu.py: the feature front-end is the
    host code with the most index arithmetic).  CPU only; never shipped."""
    out = os.path.join(HERE, "build", "pm_cli_san")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    deps = HOST_SRCS + [os.path.join(HOST_DIR, "pm_features.hpp"), os.path.join(ROOT, "include", "pm.h"), LIB]
    if any(_newer(d, out) for d in deps):
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + HOST_DIR] + HOST_SRCS + \
              ["-o", out, "-L" + HERE, "-lpm_hip", "-Wl,-rpath," + HERE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("sanitized host build failed:\n%s\n%s" % (" ".join(cmd), r.stderr))
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
    print(build_host(force="--force" in sys.argv))
