#!/usr/bin/env python3
"""Do two builds of this library WRITE the same for a scene?  Needs no GPU and compiles no module.

tools/code_identity.py compares code objects, and pays hipRTC for each: it reaches six scenes.  This compares what goes INTO hipRTC
and into the interpreter — the scene module's source, the structure module's with and without samples, the two macro-op lists —
through tools/spec_source.cpp, which calls lol_codegen.hip's generators directly, over every scene tests/scene_shapes.py makes and
every way the generator can be asked: a few thousand texts in a minute.

    python tools/source_identity.py --parent ../parent --work /tmp/srcident --out profiles/r25_source_identity.json [--sanitize]

Both trees are built already (`make` in loltracer_amd/csrc: the program links against lib/obj/*.o).  The configurations are each
varied alone against DEFAULT below.  Before the comparison is trusted the PARENT's texts are held to COVERAGE: every branch of the
emitter must have written at least one of them.  --sanitize: lol_codegen.hip and the program once more with AddressSanitizer and
UBSan on the host side (a stand-alone program on the CPU: nothing is loaded into python, nothing runs on a GPU), the whole corpus
and the program's --selftest through that, clean and with the same output.  Exit status 1 when anything differs or is not covered.
"""
import argparse
import concurrent.futures
import glob
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXAMPLES = ("scene", "scene2", "scene3", "scene4")
KINDS = ("source", "structure", "structure_samples", "lists")
MAX_JOBS = 16
MAX_FUNCTION_LINES = 120              # of the emitter in lol_codegen.hip (shape)

# the fast paths as lol_gpu_compile_offline_module assumes them (its assume_fast = 1: sqrt_kind 3), culling on, the form by size, no switch
DEFAULT = ["--assume-fast", "3", "--cull", "1", "--form", "0", "--switches", "0"]


def configurations():
    """(name, the program's arguments, the environment beside them)"""
    def but(option, value=None):
        a = list(DEFAULT)
        if value is None:
            return a + [option]
        a[a.index(option) + 1] = value
        return a
    c = [("default", DEFAULT, {}),
         ("fast paths: none", but("--assume-fast", "0"), {}),
         ("fast paths: sqrt_kind 1", but("--assume-fast", "1"), {}),
         ("fast paths: sqrt_kind 2", but("--assume-fast", "2"), {}),
         ("fast paths: sqrt_tiny_ok off", but("--no-tiny"), {}),
         ("fast paths: div_ok without div_nf_ok", but("--no-nf"), {}),
         ("fast paths: shade_root 0", but("--no-shade"), {}),
         ("culling off", but("--cull", "0"), {}),
         ("form 1 (out of line)", but("--form", "1"), {}),
         ("form 2 (inlined)", but("--form", "2"), {}),
         ("module switches: all", but("--switches", "127"), {})]
    for var, values in (("LOL_GPU_CULL_CARRY", "01"), ("LOL_GPU_CULL_VALUE_CARRY", "0"), ("LOL_GPU_CULL_UPDATE_GATED", "0"), ("LOL_GPU_CULL_KEEP", "0"),
                        ("LOL_GPU_LAST_STEP_ID", "0"),
                        ("LOL_GPU_SAT_CULL_MIN_PRIMS", "02"), ("LOL_GPU_CULL_CLUSTERS", "02"), ("LOL_GPU_INTERP_FUSE_POPS", "0"),
                        ("LOL_GPU_SPEC_INLINE_MAX", ["16"])):
        c += [("%s=%s" % (var, v), DEFAULT, {"LOL_GPU_TUNING": "1", var: v}) for v in values]
    return c


# what each branch of the emitter leaves in a text (all of a tuple in ONE text; any of a list)
COVERAGE = (
    ("out of line", "source", ("_fn(",)),
    ("the parameter form", "structure", ("K[",)),
    ("eval_rec", "source", ("eval_rec(",)),
    ("the cluster carry", "source", ("need", "lb = __builtin_fmaf(")),
    ("the value carry", "source", ("lb = maxf_(",)),
    ("spheres without range tracker", "source", ("sd_sphere_fast_nr<",)),
    ("smooth minimum of two finite-or-NaN operands", "source", ("sminf_fastdiv_sat2",)),
    ("smooth minimum without v_div_fixup", "source", ["sminf_fastdiv<false>", "sminf_fastdiv_sat<false>"]),
    ("the saturation test", "source", ("vote(!(sw",)),
    ("the tie rule", "source", ("best_id > ",)),
    ("a plain smooth minimum", "source", (" sminf_(",)),
    ("two tests guarding one run", "source", ("| vote(!(cl1",)),
)


def covered(needles, text):
    return any(n in text for n in needles) if isinstance(needles, list) else all(n in text for n in needles)


def corpus():
    """{name: .lol text}: the example scenes, everything tests/scene_shapes.py makes, and balanced trees whose union operands have 32
    and 64 primitives (so that the saturation test is written under the default threshold)"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import scene_shapes as C
    texts = {"example-" + n: open(os.path.join(C.SCENES_DIR, n + ".lol")).read() for n in EXAMPLES}
    for shape in C.RUNG_SHAPES + [C.MID, C.BIG]:
        texts["shape-" + shape.name] = shape.text()
    texts.update(("fuzz%d" % i, t) for i, t in enumerate(C.fuzz_texts()))
    texts.update(("degenerate-" + n, t) for n, t in zip(C.DEGENERATE_NAMES, C.DEGENERATE_CASES))
    texts.update(("hostile-" + e.name, e.text) for e in C.HOSTILE)
    texts.update(("compact-tree%d" % d, C.compact_tree_text(d)) for d in (6, 7))
    return texts


def makefile_flags(tree):
    csrc = os.path.join(tree, "loltracer_amd", "csrc")
    return subprocess.run(["make", "-s", "-C", csrc, "--eval", "print-flags: ; @echo $(HIPFLAGS)", "print-flags"],
                          check=True, stdout=subprocess.PIPE, text=True).stdout.split()


def build_program(tree, out, sanitize=False):
    """tools/spec_source.cpp of THIS checkout against `tree`'s headers and objects (two commands: see the program's head)"""
    csrc, lib = os.path.join(tree, "loltracer_amd", "csrc"), os.path.join(tree, "loltracer_amd", "lib")
    objs = sorted(glob.glob(os.path.join(lib, "obj", "*.o")))
    if not objs:
        raise SystemExit("%s is not built (make -C loltracer_amd/csrc)" % tree)
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    if sanitize:                                                   # lol_codegen.hip a second time, beside the tree's own object
        mine = out + ".lol_codegen.o"
        subprocess.run([HIPCC] + makefile_flags(tree) + san + ["-c", "-o", mine, "lol_codegen.hip"], cwd=csrc, check=True)
        objs = [o for o in objs if os.path.basename(o) != "lol_codegen.o"] + [mine]
    subprocess.run([HIPCC, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(tree, "include"), "-I" + csrc] + san +
                   ["-c", "-o", out + ".o", os.path.join(ROOT, "tools", "spec_source.cpp")], check=True)
    subprocess.run([HIPCC, "-o", out, out + ".o"] + objs + (["-fsanitize=address,undefined"] if sanitize else []) +
                   ["-L" + lib, "-llol_scene", "-lhiprtc", "-ldl", "-Wl,-rpath," + lib], check=True)
    return out


def run(program, args, env, files):
    e = dict(os.environ, **env)
    for k in [k for k in e if k.startswith("LOL_GPU_") and k not in env]:
        del e[k]
    r = subprocess.run([program] + list(args) + files, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit("%s %s: exit status %d\n%s" % (program, " ".join(args), r.returncode, r.stderr[-4000:]))
    return r.stdout


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def shape(tree):
    """lol_codegen.hip by the line: its length, the longest function of the SDF emitter — from `struct SdfForm`, or where there is none
    from emit_sdf's own first line, to emit_sdf's closing brace — and what must not stand in it"""
    lines = open(os.path.join(tree, "loltracer_amd", "csrc", "lol_codegen.hip"), encoding="utf-8").read().split("\n")
    at = lambda prefix, start=0: next(i for i in range(start, len(lines)) if lines[i].startswith(prefix))      # noqa: E731
    close = lambda i, indent="": next(j for j in range(i, len(lines)) if lines[j].startswith(indent + "}"))       # noqa: E731
    code = lambda x: re.sub(r"\s*/\*.*?\*/\s*$", "", x).rstrip()      # noqa: E731 (a line without the comment that ends it)
    entry = at("void emit_sdf(")
    first = at("struct SdfForm") if any(x.startswith("struct SdfForm") for x in lines) else entry
    longest, i = (0, ""), first
    while i <= close(entry):
        indent = lines[i][:len(lines[i]) - len(lines[i].lstrip("\t"))]
        word = lines[i].strip()
        # a function's first line: at file scope or one level inside a struct, no statement, no comment, no type's head
        if len(indent) <= 1 and "(" in word and word[0].isalpha() and not word.startswith(("struct ", "enum ", "if ", "for ", "return ")):
            opens = next(j for j in range(i, len(lines)) if code(lines[j]).endswith(("{", ";", "}")))
            if code(lines[opens]).endswith("{"):
                end = close(opens + 1, indent)
                longest = max(longest, (end - i + 1, word.split("(")[0].split()[-1]))
                i = end
        i += 1
    generators = lines[first:close(at("std::string generate_structure_source(")) + 1]
    return {"lines": len(lines) - 1, "longest_function_of_the_emitter": {"lines": longest[0], "name": longest[1]},
            "snprintf_from_emit_sdf_to_generate_structure_source": sum("snprintf(" in x and "vsnprintf(" not in x for x in generators),
            "std_function": sum("std::function" in x for x in lines)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", required=True, help="a built checkout of the commit to compare with")
    ap.add_argument("--work", required=True, help="directory for the programs and the corpus")
    ap.add_argument("--out", help="the JSON record")
    ap.add_argument("--sanitize", action="store_true", help="also run everything through a build with ASan and UBSan on the host side")
    ap.add_argument("--jobs", type=int, default=MAX_JOBS)
    a = ap.parse_args()
    jobs = max(1, min(a.jobs, MAX_JOBS))
    os.makedirs(os.path.join(a.work, "corpus"), exist_ok=True)
    texts = corpus()
    files = []
    for name, text in sorted(texts.items()):
        files.append(os.path.join(a.work, "corpus", name + ".lol"))
        with open(files[-1], "w") as fh:
            fh.write(text)
    names = [os.path.basename(f)[:-4] for f in files]
    old = build_program(os.path.abspath(a.parent), os.path.join(a.work, "spec_source_parent"))
    new = build_program(ROOT, os.path.join(a.work, "spec_source_this"))
    configs = configurations()
    pool = concurrent.futures.ThreadPoolExecutor(jobs)

    def hashes(program):
        """[{(scene, kind): (sha256, size)}] per configuration"""
        outs = list(pool.map(lambda c: run(program, c[1], c[2], files), configs))
        table = []
        for out in outs:
            rows = [line.rsplit(" ", 3) for line in out.splitlines()]
            table.append({(os.path.basename(f)[:-4], kind): (h, int(n)) for f, kind, h, n in rows})
            assert len(table[-1]) == len(KINDS) * len(files), "a text is missing"
        return table

    # ---- the parent's texts cover the emitter, or the comparison proves little
    counts = {what: 0 for what, _, _ in COVERAGE}
    for kind in ("source", "structure"):
        jobs_ = [(c, f) for c in configs for f in files] if kind == "source" else [(configs[0], f) for f in files]
        for text in pool.map(lambda cf: run(old, list(cf[0][1]) + ["--text", kind], cf[0][2], [cf[1]]), jobs_):
            for what, where, needles in COVERAGE:
                if where == kind and covered(needles, text):
                    counts[what] += 1
    uncovered = sorted(w for w, n in counts.items() if n == 0)

    # ---- every text and every list, by hash
    was, now = hashes(old), hashes(new)
    differing, record_configs = [], []
    for (name, args, env), x, y in zip(configs, was, now):
        bad = sorted("%s: %s: %s" % (name, scene, kind) for (scene, kind) in x if x[(scene, kind)] != y.get((scene, kind)))
        differing += bad
        record_configs.append({
            "name": name, "arguments": " ".join(args), "environment": env,
            "texts": sum(k[1] != "lists" for k in y), "lists": sum(k[1] == "lists" for k in y), "identical": not bad,
            "sha256_of_all": sha("\n".join("%s %s %s" % (s, k, y[(s, k)][0]) for s, k in sorted(y))),
            "source_and_lists_sha256_16": {s: [y[(s, "source")][0][:16], y[(s, "lists")][0][:16]] for s in names},
        })
    # ---- the shape of the file that writes them: no function of the emitter beyond 120 lines, nothing formatted into a fixed buffer
    shapes = {"parent": shape(os.path.abspath(a.parent)), "this": shape(ROOT)}
    mine = shapes["this"]
    if mine["longest_function_of_the_emitter"]["lines"] > MAX_FUNCTION_LINES or mine["std_function"] or \
       mine["snprintf_from_emit_sdf_to_generate_structure_source"]:
        differing.append("the shape of lol_codegen.hip: %s" % json.dumps(mine))
    head = lambda tree: subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], stdout=subprocess.PIPE, text=True).stdout.strip()
    record = {
        "what": "what lol_codegen.hip writes for a scene — module source, structure source with and without samples, the two macro-op "
                "lists — in this change and in its parent commit, compared by SHA-256 on a machine without a GPU (tools/source_identity.py)",
        "parent_commit": head(a.parent),
        "scenes": names, "n_scenes": len(names),
        "n_configurations": len(configs),
        "n_texts_compared": sum(c["texts"] for c in record_configs), "n_lists_compared": sum(c["lists"] for c in record_configs),
        "coverage_of_the_parents_texts": {"what": "in how many of the parent's texts each branch of the emitter shows", "counts": counts,
                                          "uncovered": uncovered},
        "identical": not differing and not uncovered, "differing": differing,
        "lol_codegen_hip": shapes,
        "default_module_source_bytes": {s: now[0][(s, "source")][1] for s in names},
        "structure_sha256_16": {s: [now[0][(s, "structure")][0][:16], now[0][(s, "structure_samples")][0][:16]] for s in names},
        "configurations": record_configs,
    }

    # ---- once more under the sanitizers: clean, and the same output
    if a.sanitize:
        san = build_program(ROOT, os.path.join(a.work, "spec_source_sanitized"), sanitize=True)
        selftest = subprocess.run([san, "--selftest"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        same = hashes(san) == now
        record["sanitized"] = {"what": "lol_codegen.hip and tools/spec_source.cpp built with -fsanitize=address,undefined on the host side, "
                                       "linked as a stand-alone program and run on the CPU over the same scenes and configurations",
                               "selftest": selftest.stdout.strip().splitlines()[-1:], "selftest_exit_status": selftest.returncode,
                               "runs": len(configs), "clean": True, "same_output": same}
        if selftest.returncode != 0 or not same:
            record["identical"] = False
            differing.append("the sanitized build")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(record, fh, indent=1)
            fh.write("\n")
    print("coverage:", ", ".join("%s %d" % kv for kv in counts.items()))
    if uncovered:
        print("NOT COVERED by any of the parent's texts:", ", ".join(uncovered))
    print("identical" if not differing else "DIFFERING:\n  " + "\n  ".join(differing[:40]))
    print("%d scenes, %d configurations: %d texts and %d lists compared" % (len(names), len(configs), record["n_texts_compared"],
                                                                           record["n_lists_compared"]))
    if a.sanitize:
        print("sanitized build:", record["sanitized"]["selftest"], "same output" if record["sanitized"]["same_output"] else "OTHER OUTPUT")
    return 0 if record["identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
