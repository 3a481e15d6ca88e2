#!/usr/bin/env python3
"""Do two builds of this library make the same device code?  Needs no GPU.

Compares this checkout with another built checkout of the repository (`--parent TREE`, `make` already run in its
loltracer_amd/csrc) and writes what was compared, and the result, as JSON:

  scene modules      for the four example scenes and the mid-size scene of tests/scene_shapes.py in both of its forms, each module
                     switch on its own plus the query kernel beside all the others, with and without assume_fast: the contents
                     of .text, .rodata and .note of the hipRTC code object — what lol_gpu_kernel_key covers — must be equal.
  ahead of time      the six .hip units compiled device-only with the Makefile's flags in both trees: every kernel's bytes and
                     its .kd descriptor (but the code's offset from it, a position in the file) must be equal, by name; kernels only
                     this checkout has are listed as `added`.
  every mask         with --masks: scene4's module for each of the 128 sets of module switches, through lol_gpu_compile_offline_shade
                     (the one call that reaches them all): the generated source and the loaded sections must be equal.

    python tools/code_identity.py --parent ../parent --work /tmp/ident --out profiles/r14_code_identity.json

`--work DIR/parent` is kept and reused when it is there, so a second run only compiles this checkout again.  Exit status 1 when
anything differs, but the modules of the scenes named by `--expect-changed`.
"""
import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("scene", "scene2", "scene3", "scene4")
# (name, lol_gpu_compile_offline_rays' enable, its mask of the other switches): the module of each lol_gpu_compile_offline* call
MODULES = (("compile_offline", 0, 0), ("_samples", 0, 2), ("_views", 0, 4), ("_view_samples", 0, 8), ("_view_blends", 0, 1),
           ("_view_blend_samples", 0, 16), ("_rays+all", 1, 31))
LOADED = (".text", ".rodata", ".note")
UNITS = ("lol_gpu", "lol_tiers", "lol_proofs", "lol_codegen", "lol_sched", "lol_multi")
N_MASKS = 128                         # seven module switches
MAX_JOBS = 16


# ---------------------------------------------------------------- ELF64 little-endian, as much as is needed
def sections(data):
    """{name: (type, flags, addr, offset, size)}"""
    shoff, = struct.unpack_from("<Q", data, 40)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 58)
    raw = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = data[raw[shstrndx][4]:raw[shstrndx][4] + raw[shstrndx][5]]
    return {names[r[0]:names.index(b"\0", r[0])].decode(): (r[1], r[2], r[3], r[4], r[5]) for r in raw}


def section_bytes(data, sec):
    return data[sec[3]:sec[3] + sec[4]]


def kernels(data):
    """{kernel: (its instructions, its descriptor)} for every symbol NAME that has a NAME.kd beside it"""
    secs = sections(data)
    shoff, = struct.unpack_from("<Q", data, 40)
    shentsize, shnum, _ = struct.unpack_from("<HHH", data, 58)
    raw = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    symtab, strtab = secs[".symtab"], secs[".strtab"]
    names = section_bytes(data, strtab)
    syms = {}
    for at in range(symtab[3], symtab[3] + symtab[4], 24):
        name, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", data, at)
        if 0 < shndx < shnum:
            sec = raw[shndx]
            syms[names[name:names.index(b"\0", name)].decode()] = data[sec[4] + value - sec[3]:sec[4] + value - sec[3] + size]
    # kernel_code_entry_byte_offset (bytes 16 ... 23 of a descriptor) is where the code lies relative to the descriptor: a position in
    # the file, which moves for every kernel of a unit when the unit gains one.  Everything else a descriptor holds is compared.
    entry = lambda kd: kd[:16] + bytes(8) + kd[24:]      # noqa: E731
    return {n: (syms[n], entry(syms[n + ".kd"])) for n in syms if n + ".kd" in syms}


def sha(b):
    return hashlib.sha256(b).hexdigest()[:16]


# ---------------------------------------------------------------- one build's code objects
def emit_modules(tree, out_dir):
    """(worker) every scene module of the build in `tree`, through that tree's own Python mirror, into out_dir"""
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    from loltracer_amd import gpu, scene as S
    import scene_shapes as C
    progs = [(n, S.Scene.parse_file(os.path.join(tree, "tests", "golden", "scenes", n + ".lol")).flatten(), 0) for n in SCENES]
    mid = C.scene_of(C.MID).flatten()
    progs += [("mid_form1", mid, 1), ("mid_form2", mid, 2)]
    want = os.environ.get("CODE_IDENTITY_ONLY")
    lib = gpu.gpu_lib()
    for name, prog, form in progs:
        if want and name != want:
            continue
        for module, enable, others in MODULES:
            for fast in (0, 1):
                base = os.path.join(out_dir, "%s.%s.fast%d" % (name, module, fast))
                st = lib.lol_gpu_compile_offline_rays(prog, b"gfx950", os.fsencode(base), fast, enable, others, form, None, 0)
                if st != 0:
                    raise SystemExit("%s: compile failed (%d)" % (base, st))


def emit_masks(tree, out_dir, part, parts):
    """(worker) scene4's module for every `parts`-th mask from `part` on, through that tree's lol_gpu_compile_offline_shade"""
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    from loltracer_amd import gpu, scene as S
    prog = S.Scene.parse_file(os.path.join(tree, "tests", "golden", "scenes", "scene4.lol")).flatten()
    lib = gpu.gpu_lib()
    for mask in range(part, N_MASKS, parts):
        # the mask's bits in the order of the switches (1 samples > 1, 2 view batches, 4 view samples, 8 view blends, 16 blend samples,
        # 32 ray queries, 64 shading queries) as that call takes them: `enable` and `others` = 1 view blends, 2 samples > 1, ...
        enable, others = mask >> 6, (mask & 0x30) | (mask & 7) << 1 | (mask >> 3 & 1)
        base = os.path.join(out_dir, "mask%03d" % mask)
        st = lib.lol_gpu_compile_offline_shade(prog, b"gfx950", os.fsencode(base), 0, enable, others, 0, None, 0)
        if st != 0:
            raise SystemExit("%s: compile failed (%d)" % (base, st))


def run_workers(commands, jobs):
    env = dict(os.environ, LOL_GPU_CACHE_DIR="")               # no disk cache: every module is really compiled
    env.pop("LOL_GPU_LIB", None)
    running = []
    for args, extra in commands:                                # the scene compiler runs one module at a time per process
        running.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + args, env=dict(env, **extra)))
        if len(running) >= jobs and running.pop(0).wait() != 0:
            raise SystemExit("a worker failed")
    if any(p.wait() != 0 for p in running):
        raise SystemExit("a worker failed")


def compile_modules(tree, out_dir, jobs):
    os.makedirs(out_dir, exist_ok=True)
    run_workers([(["--emit", out_dir, "--parent", tree], {"CODE_IDENTITY_ONLY": n}) for n in list(SCENES) + ["mid_form1", "mid_form2"]], jobs)


def compile_masks(tree, out_dir, jobs):
    os.makedirs(out_dir, exist_ok=True)
    run_workers([(["--emit-masks", out_dir, "--parent", tree, "--part", "%d/%d" % (i, jobs)], {}) for i in range(jobs)], jobs)


def loaded_sha(data):
    secs = sections(data)
    return sha(b"".join(section_bytes(data, secs[s]) for s in LOADED))


def compile_ahead_of_time(tree, out_dir):
    """the six units with the Makefile's own flags, device side only, as plain code objects"""
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(tree, "loltracer_amd", "csrc")
    flags = subprocess.run(["make", "-s", "-C", csrc, "--eval", "print-flags: ; @echo $(HIPCC) $(HIPFLAGS)", "print-flags"],
                           check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    subprocess.run(["make", "-s", "-C", csrc, "lol_kernel_src.inc", "lol_build_id.inc"], check=True)
    running = [subprocess.Popen(flags + ["--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", os.path.join(out_dir, u + ".aot.co"), u + ".hip"],
                                cwd=csrc) for u in UNITS]
    if any(p.wait() != 0 for p in running):
        raise SystemExit("hipcc failed")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--emit", help=argparse.SUPPRESS)
    ap.add_argument("--emit-masks", help=argparse.SUPPRESS)
    ap.add_argument("--part", help=argparse.SUPPRESS)
    ap.add_argument("--masks", action="store_true", help="also compare scene4's module for every set of module switches")
    ap.add_argument("--parent", help="a built checkout of the commit to compare with")
    ap.add_argument("--work", help="directory for the code objects")
    ap.add_argument("--out", help="the JSON record")
    ap.add_argument("--jobs", type=int, default=6)
    ap.add_argument("--expect-changed", default="", help="comma-separated scenes whose modules are meant to differ: they are recorded "
                    "as `changed_as_expected`, and only a difference anywhere else counts")
    ap.add_argument("--compare-only", action="store_true", help="compile nothing: compare what --work holds")
    a = ap.parse_args()
    if a.emit:
        return emit_modules(a.parent, a.emit)
    if a.emit_masks:
        return emit_masks(a.parent, a.emit_masks, *map(int, a.part.split("/")))
    a.jobs = max(1, min(a.jobs, MAX_JOBS))
    old, new = os.path.join(a.work, "parent"), os.path.join(a.work, "this")
    if not a.compare_only:
        if not os.path.exists(os.path.join(old, "lol_gpu.aot.co")):
            compile_ahead_of_time(os.path.abspath(a.parent), old)
        if not os.path.exists(os.path.join(old, "scene.compile_offline.fast0.co")):
            compile_modules(os.path.abspath(a.parent), old, a.jobs)
        compile_ahead_of_time(ROOT, new)
        compile_modules(ROOT, new, a.jobs)
        if a.masks:
            if not os.path.exists(os.path.join(old, "masks", "mask%03d.co" % (N_MASKS - 1))):
                compile_masks(os.path.abspath(a.parent), os.path.join(old, "masks"), a.jobs)
            compile_masks(ROOT, os.path.join(new, "masks"), a.jobs)

    def read(d, f):
        with open(os.path.join(d, f), "rb") as fh:
            return fh.read()

    differing, modules, units = [], [], []
    files = sorted(f for f in os.listdir(old) if f.endswith(".co"))
    assert files == sorted(f for f in os.listdir(new) if f.endswith(".co")), "the two builds wrote different sets of modules"
    for f in files:
        x, y = read(old, f), read(new, f)
        if f.endswith(".aot.co"):
            kx, ky = kernels(x), kernels(y)
            bad = sorted(n for n in kx if kx[n] != ky.get(n))               # every kernel the other build has; new ones are listed, not compared
            units.append({"unit": f[:-len(".aot.co")] + ".hip", "kernels": len(ky), "added": sorted(set(ky) - set(kx)),
                          "sha256_16_of_all": sha(b"".join(n.encode() + b"\0" + ky[n][0] + ky[n][1] for n in sorted(ky))), "differing": bad})
            differing += [f + ": " + n for n in bad]
        else:
            sx, sy = sections(x), sections(y)
            rec = {"module": f[:-3], "file_bytes_differing": sum(p != q for p, q in zip(x, y)) + abs(len(x) - len(y))}
            for s in LOADED:
                bx, by = section_bytes(x, sx[s]), section_bytes(y, sy[s])
                rec[s] = {"bytes": len(by), "sha256_16": sha(by), "equal": bx == by}
                if bx != by:
                    differing.append(f + ": " + s)
            rec["source_equal"] = read(old, f[:-3] + ".hip") == read(new, f[:-3] + ".hip")
            if not rec["source_equal"]:
                differing.append(f + ": generated source")
            modules.append(rec)
    masks = []
    if a.masks:
        for mask in range(N_MASKS):
            f = os.path.join("masks", "mask%03d" % mask)
            src, co = (read(old, f + ".hip"), read(new, f + ".hip")), (read(old, f + ".co"), read(new, f + ".co"))
            rec = {"mask": mask, "source_sha256_16": sha(src[1]), "loaded_sha256_16": loaded_sha(co[1]),
                   "equal": src[0] == src[1] and loaded_sha(co[0]) == loaded_sha(co[1])}
            masks.append(rec)
            if not rec["equal"]:
                differing.append(f)
    # the key of scene4's plain module (lol_gpu_kernel_key of the frames of the flagship workload), by this checkout's library
    sys.path.insert(0, ROOT)
    from loltracer_amd import gpu
    plain = "scene4.compile_offline.fast0.co"
    keys = {"parent": gpu.code_key(read(old, plain)), "this": gpu.code_key(read(new, plain))}
    if keys["parent"] != keys["this"]:
        differing.append(plain + ": code key")
    # modules that are meant to differ (--expect-changed): listed apart; the plain module's key then differs with them
    meant = tuple(n + "." for n in a.expect_changed.split(",") if n)
    expected = sorted({d.split(":")[0] for d in differing if d.startswith(meant)}) if meant else []
    differing = [d for d in differing if not (meant and d.startswith(meant))]
    head = lambda tree: subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], stdout=subprocess.PIPE, text=True).stdout.strip()
    record = {
        "what": "device code of this change against its parent commit, compared on a machine without a GPU (tools/code_identity.py)",
        "parent_commit": head(a.parent) if a.parent else None,
        "compared": {"scene_modules": "contents of .text, .rodata and .note of the hipRTC code object (gfx950), and the generated source",
                     "ahead_of_time": "every kernel's bytes and its .kd descriptor, by name, of each .hip unit compiled device-only with the Makefile's flags"},
        "scenes": list(SCENES) + ["scene_shapes.MID form 1", "scene_shapes.MID form 2"],
        "modules": [m[0] for m in MODULES], "assume_fast": [0, 1],
        "n_scene_modules": len(modules), "n_ahead_of_time_kernels": sum(u["kernels"] for u in units),
        "identical": not differing, "differing": differing, "changed_as_expected": expected,
        "scene4_plain_module_code_key": keys,
        "scene_modules": modules, "ahead_of_time_units": units,
    }
    if a.masks:
        record["every_mask"] = {"what": "scene4's module for each set of module switches (bit values: include/lol_gpu_diag.h, "
                                        "lol_gpu_compile_offline_module), assume_fast 0, through lol_gpu_compile_offline_shade in both trees: "
                                        "SHA-256 of the generated source and of .text + .rodata + .note",
                                "n": len(masks), "n_equal": sum(m["equal"] for m in masks), "masks": masks}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(record, fh, indent=1)
            fh.write("\n")
    print("identical" if not differing else "DIFFERING:\n  " + "\n  ".join(differing[:40]))
    print("%d scene modules, %d ahead-of-time kernels" % (len(modules), record["n_ahead_of_time_kernels"]))
    if a.masks:
        print("%d of %d masks equal" % (record["every_mask"]["n_equal"], len(masks)))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
