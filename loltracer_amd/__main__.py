"""python -m loltracer_amd scene.lol [-o frame.ppm] [--size WxH] [--max-steps N] [--device D] [--frames N] [--samples N]
                          [--adaptive T] [--orbit K -o DIR [--orbit-samples N [--orbit-adaptive T]] [--orbit-shutter K]]
                          [--lens R (--focus D | --focus-at X,Y) --lens-samples K] [--pick X,Y] [--panorama WxH -o FILE.ppm]
                          [--tween B.lol --frames N [--tween-samples S] [--tween-shutter K] -o DIR]
                          [--tween B.lol --frames N --pick X,Y] [--tween B.lol --frames N --lens R --focus-at X,Y [--lens-samples K] -o DIR]
                          [--relight LOOK.lol [LOOK2.lol ...] [--samples S] [--lens R --focus D --lens-samples K] [--move-lights] -o DIR]
                          [--tween B.lol --frames N --relight LOOK.lol [LOOK2.lol ...] [--tween-samples S] -o DIR]

Renders a `.lol` scene on the GPU through the C ABI (liblol_gpu.so) and writes a binary PPM — the Python spelling of
`loltracer_amd/lib/lol_headless`.  With --orbit K it renders K views from a circle round the scene (scene.orbit_cameras) as ONE batch
(Renderer.render_views_into) and writes DIR/view_0000.ppm ...; --orbit-samples N supersamples the views of that batch (N x N samples
per pixel; with --orbit-adaptive T only at the edges of each view); --orbit N --orbit-shutter K blurs each of the N views by the motion
inside its own exposure: view v is the mean in linear light of cameras v K ... v K + K - 1 of scene.orbit_cameras(scene, N K)
(Renderer.render_blended_views_into); with --orbit-samples S beside it every one of those cameras is supersampled S x S (not with
--orbit-adaptive).  --lens R --focus D --lens-samples K renders ONE frame with depth of field: the mean over the K cameras of
scene.lens_cameras on a lens of radius R focused at distance D; with --samples S every lens camera is supersampled S x S (not with
--adaptive); --focus-at X,Y in the place of --focus D is autofocus: D is the distance, along the camera's axis, of what pixel
(X, Y) shows (one Renderer.pick; refused when that ray escapes).  --pick X,Y prints the object id, distance, step count and normal
under pixel (X, Y) of the --size frame (one ray, Renderer.pick); no frame is rendered unless -o is also given.  --panorama WxH
writes the equirectangular image of everything round the camera's position: the rays of scene.panorama_rays shaded by ONE shading
query (Renderer.shade_rays_into) — rays of the host's own making, the reference's colours.  A.lol --tween B.lol --frames N renders
the N frames of an animation from scene A to scene B (same structure, other numbers: scene.tween) in ONE launch, every frame under a
scene of its own (Renderer.render_scene_views_into), and writes DIR/frame_0000.ppm ...; with --tween-shutter K each frame is the mean
in linear light of K scenes spread over its exposure (scene.shutter_times): objects that move are blurred; with --tween-samples S
every one of those scenes is supersampled S x S (the samples= of that call; --samples stays refused beside --tween: it is the frame
setting of a context, which that call does not read).  The camera is A's.  --pick X,Y beside --tween prints one pick line per
frame, in --pick's format, from ONE scene query over the frames' scenes (Renderer.pick_scenes; no -o needed), and --lens R --focus-at
X,Y [--lens-samples K] beside --tween pulls focus: frame f is the mean over the K lens cameras focused at what pixel (X, Y) shows IN
FRAME f (its pick times the cosine to the camera's axis), K records of that frame's scene in the same one launch; a frame whose ray
hits nothing is an error that names the frame; not with --tween-shutter.  SCENE.lol --relight LOOK.lol [LOOK2.lol ...] -o DIR
captures the light passes of every pixel of the --size frame ONCE (Renderer.light_pixels_into) and makes one frame per look from them
without marching again (Renderer.relight_into): DIR/look_0000.ppm ... are the frames of the looks' scenes, byte for byte.  A look is
the scene with other light intensities, material colours or ambient colour (scene.same_geometry); one that differs in anything else
is refused with its first difference.  The camera is SCENE's.  With --samples S, or --lens R --focus D --lens-samples K [--samples S],
beside --relight the looks are AVERAGED frames: every sample under every lens camera is captured once (Renderer.light_views_into: one
capture per camera) and each look is resolved in linear light before gamma (Renderer.relight_views_into) — the files LOOK.lol with
the same flags and without --relight writes, byte for byte.  Not with --adaptive or --focus-at.  With --move-lights beside --relight
the looks may also MOVE LIGHTS or change a shininess: each look is reached from the one before by scene.light_changes, one light update
(Renderer.light_update_pixels_into: no primary march, a shadow march only towards lights that moved) and relight_into(held=look);
the files are again what LOOK.lol alone writes, byte for byte.  Not with --samples, --lens, --adaptive or --focus-at.
A.lol --tween B.lol --frames N --relight LOOK.lol [LOOK2.lol ...] -o DIR relights an ANIMATION: ONE capture over the N tweened scenes
(Renderer.light_scene_pixels_into: every frame under its own scene, one launch) and per look ONE Renderer.relight_scenes_into, frame
f under its own scene with the look's intensities and colours (look_of: scene.Scene.with_look from the look's file), into
DIR/look_LLLL_frame_FFFF.ppm — the frames those scenes render, byte for byte.  With --tween-samples S beside it the frames are
SUPERSAMPLED: the one capture takes every sample of every frame (the S w x S h grid of each scene) and each look is ONE
Renderer.relight_scene_views_into, averaged in linear light before gamma — the files --tween B.lol --tween-samples S writes of the
look's scenes, byte for byte.  Not with --tween-shutter (the blurred form is reached from Python: cameras_per_view=K), --samples,
--lens or --move-lights.
There is no CPU rendering path."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

from . import gpu, scene as S


def write_ppm(path, surf):
    rgb = np.stack([(surf >> 16) & 0xFF, (surf >> 8) & 0xFF, surf & 0xFF], axis=-1).astype(np.uint8)
    with open(path, "wb") as fp:
        fp.write(b"P6\n%d %d\n255\n" % (surf.shape[1], surf.shape[0]))
        fp.write(rgb.tobytes())


def orbit(sc, args, w, h) -> int:
    """K views of one batch into K PPMs"""
    k, shutter = args.orbit, args.orbit_shutter
    r = gpu.Renderer(args.device)
    try:
        r.set_view_batches(True)             # before prepare(): the scene's own kernel then carries the batch form
        if args.orbit_samples > 1 and shutter == 1:
            r.set_view_samples(True)         # ... and the supersampled batch forms
        if shutter > 1 and args.orbit_samples == 1:
            r.set_view_blends(True)          # ... and the linear-colour form of blends
        if shutter > 1 and args.orbit_samples > 1:
            r.set_view_blend_samples(True)   # ... and its supersampled form
        r.prepare(sc)
        views = np.zeros((k, h, w), dtype=np.uint32)
        dev = r.malloc(views.nbytes)
        try:
            t0 = time.perf_counter()
            if shutter > 1:
                r.render_blended_views_into(dev, S.orbit_cameras(sc, k * shutter), shutter, w, h, args.max_steps,
                                            samples=args.orbit_samples)
            else:
                r.render_views_into(dev, S.orbit_cameras(sc, k), w, h, args.max_steps, samples=args.orbit_samples,
                                    adaptive=args.orbit_adaptive if args.orbit_samples > 1 else -1)
            r.sync()
            dt = (time.perf_counter() - t0) * 1e3
            r.memcpy_d2h(views.ctypes.data, dev, views.nbytes)
        finally:
            r.free(dev)
    finally:
        r.close()
    print(f"{k} views of {w}x{h}: {dt:.3f}ms  {k * w * h / dt / 1e3:.1f} Mpixels/s")
    os.makedirs(args.out, exist_ok=True)
    for v in range(k):
        write_ppm(os.path.join(args.out, f"view_{v:04d}.ppm"), views[v])
    return 0


def tween_frames(sc, args, w, h) -> int:
    """N frames from scene A to scene B in one launch into N PPMs"""
    try:
        other = S.Scene.parse_file(args.tween)
    except S.SceneError as e:
        print(e.message, file=sys.stderr)
        return 1
    if not S.same_structure(sc, other):
        print("--tween: the two scenes differ in structure (objects, their nesting, lights or materials)", file=sys.stderr)
        return 1
    n, k = args.frames, args.tween_shutter
    scenes = [S.tween(sc, other, t) for f in range(n) for t in S.shutter_times(f, n, k)]
    cams = [sc.camera] * len(scenes)
    r = gpu.Renderer(args.device)
    try:
        # (no set_scene_views: the interpreter's kernels with the upload's proven fast paths were the faster route where both were
        # measured; a host whose scenes gain from the structure module sets it before prepare())
        queries = bool(args.pick or args.focus_at)
        r.prepare(sc, wait=not queries)      # (scene queries and the frames behind them run on the interpreter: nothing waits)
        if queries:
            # what pixel (X, Y) shows in every frame (k = 1 here): ONE scene query over the frames' scenes
            x, y = pixel_arg(args.pick or args.focus_at, w, h)
            picks = r.pick_scenes(scenes, x, y, w, h, cameras=cams, max_steps=args.max_steps)
        if args.pick:
            for p in picks:
                print(pick_line(x, y, p))
            if not args.out:
                return 0
        if args.lens:
            # a lens that follows what (X, Y) shows: frame f is the mean over the K lens cameras focused at ITS pick, K records of its scene
            k = args.lens_samples
            focus = [args.focus] * n
            if args.focus_at:
                cosine = axis_cosine(sc, w, h, x, y)
                for f, p in enumerate(picks):
                    if p["id"] == 0 or not p["dist"] > 0:
                        print(f"--focus-at {x},{y}: in frame {f} the ray of that pixel hits nothing to focus on", file=sys.stderr)
                        return 1
                    focus[f] = p["dist"] * cosine
                    print(f"frame {f}: focus at {x},{y}: object {p['id']} at {p['dist']:.6g} along its ray, {focus[f]:.6g} along the camera's axis")
            cams = [c for f in range(n) for c in S.lens_cameras(sc.camera, focus[f], args.lens, k)]
            scenes = [scenes[f] for f in range(n) for _ in range(k)]
        frames = np.zeros((n, h, w), dtype=np.uint32)
        dev = r.malloc(frames.nbytes)
        try:
            t0 = time.perf_counter()
            r.render_scene_views_into(dev, cams, scenes, w, h, k, args.max_steps, samples=args.tween_samples)
            r.sync()
            dt = (time.perf_counter() - t0) * 1e3
            r.memcpy_d2h(frames.ctypes.data, dev, frames.nbytes)
            name = r.scene_view_samples_kernel_name(k, args.tween_samples)
        finally:
            r.free(dev)
    finally:
        r.close()
    ss = args.tween_samples
    print(f"{n} frames of {w}x{h} over {k} scene(s) each{f', {ss}x{ss} samples per pixel' if ss > 1 else ''}: {dt:.3f}ms  {n * w * h / dt / 1e3:.1f} Mpixels/s  [{name}]")
    os.makedirs(args.out, exist_ok=True)
    for f in range(n):
        write_ppm(os.path.join(args.out, f"frame_{f:04d}.ppm"), frames[f])
    return 0


def relight_frames(sc, args, w, h) -> int:
    """one capture of every pixel, one relight per look, one PPM per look"""
    looks = []
    for path in args.relight:
        try:
            look = S.Scene.parse_file(path)
        except S.SceneError as e:
            print(e.message, file=sys.stderr)
            return 1
        why = S.geometry_difference(sc, look, lighting=not args.move_lights)
        if why is not None:
            print(f"--relight {path}: not a look of {args.scene}: {why}", file=sys.stderr)
            return 1
        looks.append(look)
    # the leaves of the frame: s x s samples under each of the K cameras of the lens (one camera, the scene's, without --lens)
    s, k = args.samples, args.lens_samples if args.lens else 1
    cams = S.lens_cameras(sc.camera, args.focus, args.lens, k) if args.lens else [sc.camera]
    averaged = s > 1 or k > 1
    n, nl = k * s * s * w * h, len(sc.lights())
    r = gpu.Renderer(args.device)
    try:
        r.prepare(sc, wait=False)            # (the capture runs on the interpreter: nothing waits for the scene compiler)
        frames = np.zeros((len(looks), h, w), dtype=np.uint32)
        d_factors = r.malloc(16 * n * nl) if nl else 0
        d_id, d_px = r.malloc(4 * n), r.malloc(4 * w * h)
        d_dist = r.malloc(4 * n) if args.move_lights else 0       # an update reads the march's distance back
        held = sc                                                 # what the planes hold: each look is reached from the one before
        try:
            t0 = time.perf_counter()
            if averaged:
                r.light_views_into(cams, k, w, h, s, args.max_steps, factors_ptr=d_factors, id_ptr=d_id)
            else:
                r.light_pixels_into(n, w, h, args.max_steps, factors_ptr=d_factors, id_ptr=d_id, dist_ptr=d_dist)
            r.sync()
            capture_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            for i, look in enumerate(looks):
                if averaged:
                    r.relight_views_into(look, 1, k, w, h, s, factors_ptr=d_factors, id_ptr=d_id, pixel_ptr=d_px)
                elif args.move_lights:
                    march, specular = S.light_changes(held, look)
                    r.light_update_pixels_into(look, n, w, h, march, specular, factors_ptr=d_factors, id_ptr=d_id, dist_ptr=d_dist)
                    r.relight_into(look, n, factors_ptr=d_factors, id_ptr=d_id, pixel_ptr=d_px, held=look)
                    held = look
                else:
                    r.relight_into(look, n, factors_ptr=d_factors, id_ptr=d_id, pixel_ptr=d_px)
                r.sync()
                r.memcpy_d2h(frames[i].ctypes.data, d_px, 4 * w * h)
            dt = (time.perf_counter() - t0) * 1e3
        finally:
            for d in (d_factors, d_id, d_px, d_dist):
                if d:
                    r.free(d)
    finally:
        r.close()
    shape = f", {s}x{s} samples per pixel" * (s > 1) + f", {k} lens cameras" * (k > 1)
    print(f"{len(looks)} look(s) of {w}x{h}{shape}: capture {capture_ms:.3f}ms, relights and copies {dt:.3f}ms  "
          f"[light_interp, {'light_update_interp, ' * bool(args.move_lights)}{'relight_views' if averaged else 'relight_rays'}]")
    os.makedirs(args.out, exist_ok=True)
    for i in range(len(looks)):
        write_ppm(os.path.join(args.out, f"look_{i:04d}.ppm"), frames[i])
    return 0


def look_of(sc, look):
    """`sc` with the look of the scene `look`: its lights' intensities, its materials' colours and its ambient colour, nothing else"""
    return sc.with_look(lights=[(l.diffuse_intensity.tuple(), l.specular_intensity.tuple()) for l in look.lights()],
                        materials=[(m.diffuse.tuple(), m.specular.tuple(), m.ambient.tuple()) for m in look.materials()],
                        ambient=look.c.ambient_color.tuple())


def tween_relight_frames(sc, args, w, h) -> int:
    """N tweened scenes captured in one launch — every sample of every frame —, one relight over all of them per look, one PPM per look
    and frame"""
    try:
        other = S.Scene.parse_file(args.tween)
        look_files = [S.Scene.parse_file(path) for path in args.relight]
    except S.SceneError as e:
        print(e.message, file=sys.stderr)
        return 1
    if not S.same_structure(sc, other):
        print("--tween: the two scenes differ in structure (objects, their nesting, lights or materials)", file=sys.stderr)
        return 1
    for path, look in zip(args.relight, look_files):
        why = S.geometry_difference(sc, look)
        if why is not None:
            print(f"--relight {path}: not a look of {args.scene}: {why}", file=sys.stderr)
            return 1
    n, px, nl, ss = args.frames, w * h, len(sc.lights()), args.tween_samples
    leaves = ss * ss * px                    # of one frame: the ss w x ss h grid under its scene
    scenes = [S.tween(sc, other, t) for f in range(n) for t in S.shutter_times(f, n, 1)]
    cams = [sc.camera] * n
    r = gpu.Renderer(args.device)
    try:
        r.prepare(sc, wait=False)            # (capture and relight run on the interpreter: nothing waits for the scene compiler)
        frames = np.zeros((len(look_files), n, h, w), dtype=np.uint32)
        d_factors = r.malloc(16 * n * leaves * nl) if nl else 0
        d_id, d_px = r.malloc(4 * n * leaves), r.malloc(4 * n * px)
        try:
            t0 = time.perf_counter()
            r.light_scene_pixels_into(scenes, leaves, ss * w, ss * h, 0, args.max_steps, factors_ptr=d_factors, id_ptr=d_id, cameras=cams)
            r.sync()
            capture_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            for i, look in enumerate(look_files):
                # (one sample per pixel: the call forwards to relight_scenes_into's)
                r.relight_scene_views_into(scenes, [look_of(s_, look) for s_ in scenes], n, 1, w, h, ss, factors_ptr=d_factors, id_ptr=d_id,
                                           pixel_ptr=d_px)
                r.sync()
                r.memcpy_d2h(frames[i].ctypes.data, d_px, 4 * n * px)
            dt = (time.perf_counter() - t0) * 1e3
        finally:
            for d in (d_factors, d_id, d_px):
                if d:
                    r.free(d)
    finally:
        r.close()
    print(f"{len(look_files)} look(s) of {n} frames of {w}x{h}{f', {ss}x{ss} samples per pixel' if ss > 1 else ''}: capture {capture_ms:.3f}ms, "
          f"relights and copies {dt:.3f}ms  [light_interp_scenes, {'relight_views_scenes' if ss > 1 else 'relight_rays_scenes'}]")
    os.makedirs(args.out, exist_ok=True)
    for i in range(len(look_files)):
        for f in range(n):
            write_ppm(os.path.join(args.out, f"look_{i:04d}_frame_{f:04d}.ppm"), frames[i, f])
    return 0


def pixel_arg(text, w, h):
    """"X,Y" -> (x, y) inside the w x h frame, or None"""
    try:
        x, y = (int(v) for v in text.split(","))
    except ValueError:
        return None
    return (x, y) if 0 <= x < w and 0 <= y < h else None


def pick_line(x, y, p) -> str:
    """the line --pick prints (lol_headless --pick prints the same)"""
    return "pick %d,%d: id=%u dist=%.9g steps=%u normal=(%.9g, %.9g, %.9g)" % ((x, y, p["id"], p["dist"], p["steps"]) + tuple(p["normal"]))


def axis_cosine(sc, w, h, x, y) -> float:
    """the cosine between the primary ray of pixel (x, y) and the camera's direction (host arithmetic, in doubles)"""
    fc = sc.frame_camera(w, h)
    vx, vy = (x + .5) / w * 2. - 1., 1. - (y + .5) / h * 2.
    d, right, up = (np.array(v.tuple(), np.float64) for v in (fc.dir, fc.right, fc.up))
    rd = right * (vx * fc.width) + up * (vy * fc.height) + d
    return float(rd @ d / (np.linalg.norm(rd) * np.linalg.norm(d)))


def lens(sc, args, w, h) -> int:
    """one frame averaged over the cameras of a lens into one PPM"""
    r = gpu.Renderer(args.device)
    try:
        if args.samples > 1:
            r.set_view_blend_samples(True)   # before prepare(): the scene's own kernel then carries the supersampled linear form
        else:
            r.set_view_blends(True)
        r.prepare(sc)
        if args.focus_at:
            x, y = pixel_arg(args.focus_at, w, h)
            p = r.pick(x, y, w, h, args.max_steps)
            if p["id"] == 0 or not p["dist"] > 0:
                print(f"--focus-at {x},{y}: the ray of that pixel hits nothing to focus on", file=sys.stderr)
                return 1
            args.focus = p["dist"] * axis_cosine(sc, w, h, x, y)
            print(f"focus at {x},{y}: object {p['id']} at {p['dist']:.6g} along its ray, {args.focus:.6g} along the camera's axis")
        surf = np.zeros((h, w), dtype=np.uint32)
        dev = r.malloc(surf.nbytes)
        try:
            t0 = time.perf_counter()
            r.render_blended_views_into(dev, S.lens_cameras(sc.camera, args.focus, args.lens, args.lens_samples), args.lens_samples,
                                        w, h, args.max_steps, samples=args.samples)
            r.sync()
            dt = (time.perf_counter() - t0) * 1e3
            r.memcpy_d2h(surf.ctypes.data, dev, surf.nbytes)
        finally:
            r.free(dev)
    finally:
        r.close()
    print(f"{w}x{h} over {args.lens_samples} lens cameras: {dt:.3f}ms")
    if args.out:
        write_ppm(args.out, surf)
    return 0


def panorama(sc, args) -> int:
    """the equirectangular image round the camera into one PPM: one list of rays, one shading query"""
    try:
        w, h = (int(v) for v in args.panorama.lower().split("x"))
    except ValueError:
        w = h = 0
    if w < 1 or h < 1 or not args.out:
        print("--panorama takes WxH and -o FILE.ppm", file=sys.stderr)
        return 1
    rays = S.panorama_rays(sc.camera, w, h)
    r = gpu.Renderer(args.device)
    try:
        r.set_shade_queries(True)            # before prepare(): the scene's own kernel then carries the shading-query form
        r.prepare(sc)
        surf = np.zeros((h, w), dtype=np.uint32)
        d_rays, d_px = r.malloc(rays.nbytes), r.malloc(surf.nbytes)
        try:
            r.memcpy_h2d(d_rays, rays.ctypes.data, rays.nbytes)
            t0 = time.perf_counter()
            r.shade_rays_into(d_rays, len(rays), args.max_steps, pixel_ptr=d_px)
            r.sync()
            dt = (time.perf_counter() - t0) * 1e3
            r.memcpy_d2h(surf.ctypes.data, d_px, surf.nbytes)
            name = r.shade_kernel_name()
        finally:
            r.free(d_rays)
            r.free(d_px)
    finally:
        r.close()
    print(f"panorama {w}x{h}: {dt:.3f}ms  {w * h / dt / 1e3:.1f} Mrays/s  [{name}]")
    write_ppm(args.out, surf)
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m loltracer_amd", description=__doc__.split("\n\n")[1])
    ap.add_argument("scene")
    ap.add_argument("-o", "--out", default=None)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--max-steps", type=int, default=256)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frames", type=int, default=1)
    ap.add_argument("--samples", type=int, default=1, choices=(1, 2, 4), help="N x N samples per pixel (supersampling)")
    ap.add_argument("--adaptive", type=int, default=-1, metavar="T",
                    help="with --samples N: N x N samples only at edges of the plain frame (contrast T, 0 ... 255)")
    ap.add_argument("--orbit", type=int, default=0, metavar="K",
                    help="K views from a circle round the scene in one batch; -o names the directory the PPMs go to")
    ap.add_argument("--orbit-samples", type=int, default=1, choices=(1, 2, 4), metavar="N",
                    help="with --orbit: N x N samples per pixel in every view of the batch")
    ap.add_argument("--orbit-adaptive", type=int, default=-1, metavar="T",
                    help="with --orbit-samples N: N x N samples only at edges of each view (contrast T, 0 ... 255)")
    ap.add_argument("--orbit-shutter", type=int, default=1, choices=(1, 2, 4, 8, 16), metavar="K",
                    help="with --orbit N: every view is the mean of K cameras of its own exposure (motion blur)")
    ap.add_argument("--lens", type=float, default=0.0, metavar="R", help="depth of field: the radius of the lens (with --focus)")
    ap.add_argument("--focus", type=float, default=0.0, metavar="D", help="with --lens: the distance that stays sharp")
    ap.add_argument("--lens-samples", type=int, default=16, choices=(1, 2, 4, 8, 16), metavar="K",
                    help="with --lens: cameras on the lens")
    ap.add_argument("--focus-at", default=None, metavar="X,Y",
                    help="with --lens, in the place of --focus: focus on what pixel X,Y of the frame shows (autofocus)")
    ap.add_argument("--pick", default=None, metavar="X,Y",
                    help="print object id, distance, steps and normal under pixel X,Y of the --size frame; no frame unless -o is given")
    ap.add_argument("--panorama", default=None, metavar="WxH",
                    help="the equirectangular image round the camera's position, WxH pixels, through one shading query; -o names the PPM")
    ap.add_argument("--tween", default=None, metavar="B.lol",
                    help="with --frames N and -o DIR: N frames from this scene to B.lol (same structure) in one launch")
    ap.add_argument("--tween-shutter", type=int, default=1, choices=(1, 2, 4, 8, 16), metavar="K",
                    help="with --tween: every frame is the mean of K scenes of its own exposure (motion blur of moving objects)")
    ap.add_argument("--tween-samples", type=int, default=1, choices=(1, 2, 4), metavar="S",
                    help="with --tween: S x S samples per pixel under every scene of every frame")
    ap.add_argument("--relight", default=None, nargs="+", metavar="LOOK.lol",
                    help="with -o DIR: one capture of the frame's light passes, then one frame per look (same geometry, other light "
                         "intensities, material colours, ambient colour) without marching again")
    ap.add_argument("--move-lights", action="store_true",
                    help="with --relight: the looks may also move lights or change a shininess; each is reached from the one before by a "
                         "light update, without the primary march (not with --samples, --lens, --adaptive or --focus-at)")
    args = ap.parse_args(argv)
    w, h = (int(v) for v in args.size.lower().split("x"))
    for name, text in (("--pick", args.pick), ("--focus-at", args.focus_at)):
        if text is not None and pixel_arg(text, w, h) is None:
            print(f"{name} takes X,Y inside the {w}x{h} frame", file=sys.stderr)
            return 1
    if args.focus_at is not None and (not args.lens or args.focus):
        print("--focus-at X,Y goes with --lens R, in the place of --focus D", file=sys.stderr)
        return 1
    try:
        sc = S.Scene.parse_file(args.scene)
    except S.SceneError as e:
        print(e.message, file=sys.stderr)
        return 1
    if not sc.validate_materials():
        print("scene_validate_materials failed", file=sys.stderr)
        return 1
    if (args.tween_shutter != 1 or args.tween_samples != 1) and not args.tween:
        print("--tween-shutter and --tween-samples go with --tween B.lol", file=sys.stderr)
        return 1
    if args.move_lights and (not args.relight or args.samples != 1 or args.lens or args.adaptive != -1 or args.focus_at):
        print("--move-lights goes with --relight LOOK.lol ... -o DIR; not with --samples, --lens, --adaptive or --focus-at", file=sys.stderr)
        return 1
    if args.relight and args.tween:
        for flag, given, why in (
                ("--tween-shutter", args.tween_shutter != 1, "the blurred form is reached from Python (relight_scene_views_into, cameras_per_view=K)"),
                ("--samples", args.samples != 1, "it is the frame setting of a context, which the capture over scenes does not read"),
                ("--lens", bool(args.lens), "a lens is an averaged resolve over records, which relight_scenes_into does not make"),
                ("--move-lights", args.move_lights, "there is no light update over records: every look keeps its frame's light points and shininess")):
            if given:
                print(f"--tween B.lol --relight LOOK.lol ... does not go with {flag}: {why}", file=sys.stderr)
                return 1
        if (args.panorama or args.orbit or args.pick or args.focus_at or args.adaptive != -1 or not args.out or args.frames < 1
                or args.frames > gpu.MAX_VIEWS):
            print(f"--tween B.lol --relight LOOK.lol ... takes --frames N (N <= {gpu.MAX_VIEWS}) and -o DIR; not with --panorama, --orbit, "
                  "--pick, --focus-at or --adaptive", file=sys.stderr)
            return 1
        return tween_relight_frames(sc, args, w, h)
    if args.relight:
        if (args.tween or args.panorama or args.orbit or args.pick or args.focus_at or args.adaptive != -1 or args.frames != 1
                or not args.out):
            print("--relight LOOK.lol ... takes -o DIR, and --samples S or --lens R --focus D --lens-samples K for averaged frames; "
                  "not with --tween, --panorama, --orbit, --pick, --focus-at, --adaptive or --frames", file=sys.stderr)
            return 1
        if args.lens < 0 or (args.lens and not args.focus > 0) or (args.focus and not args.lens):
            print("--relight with --lens R takes a radius > 0 and --focus D > 0", file=sys.stderr)
            return 1
        return relight_frames(sc, args, w, h)
    if args.tween:
        per_frame = args.lens_samples if args.lens else args.tween_shutter
        if (args.panorama or args.orbit or args.samples != 1 or args.adaptive != -1 or not (args.out or (args.pick and not args.lens))
                or args.frames < 1 or args.frames * per_frame > gpu.MAX_VIEWS):
            print(f"--tween B.lol takes --frames N (N K <= {gpu.MAX_VIEWS} scenes with --tween-shutter K or --lens R --lens-samples K) and "
                  "-o DIR (--pick X,Y alone needs no -o); not with --panorama, --orbit, --samples or --adaptive", file=sys.stderr)
            return 1
        if args.lens and (args.lens < 0 or not (args.focus > 0 or args.focus_at) or args.pick or args.tween_shutter != 1):
            print("--tween with --lens R takes a radius > 0 and --focus-at X,Y (or --focus D > 0); not with --pick or --tween-shutter",
                  file=sys.stderr)
            return 1
        if args.pick and args.tween_shutter != 1:
            print("--tween with --pick X,Y prints one line per frame: not with --tween-shutter", file=sys.stderr)
            return 1
        return tween_frames(sc, args, w, h)
    if args.panorama:
        if args.orbit or args.lens or args.pick or args.samples != 1 or args.adaptive != -1 or args.frames != 1:
            print("--panorama does not go with --orbit, --lens, --pick, --samples, --adaptive or --frames", file=sys.stderr)
            return 1
        return panorama(sc, args)
    if args.orbit:
        if (args.orbit < 1 or args.orbit > gpu.MAX_VIEWS or args.samples != 1 or args.adaptive != -1 or args.frames != 1
                or not args.out):
            print(f"--orbit takes 1 ... {gpu.MAX_VIEWS} views and -o DIR; not with --samples, --adaptive or --frames", file=sys.stderr)
            return 1
        if args.orbit_adaptive < -1 or args.orbit_adaptive > 255:
            print("--orbit-adaptive takes a contrast 0 ... 255", file=sys.stderr)
            return 1
        if args.lens:
            print("--orbit does not go with --lens: the lens mode renders one frame", file=sys.stderr)
            return 1
        if args.orbit_shutter > 1 and args.orbit * args.orbit_shutter > gpu.MAX_VIEWS:
            print(f"--orbit N --orbit-shutter K takes N K <= {gpu.MAX_VIEWS} cameras", file=sys.stderr)
            return 1
        if args.orbit_shutter > 1 and args.orbit_samples > 1 and args.orbit_adaptive != -1:
            print("--orbit-shutter K with --orbit-samples S samples every pixel: not with --orbit-adaptive", file=sys.stderr)
            return 1
        return orbit(sc, args, w, h)
    if args.orbit_samples != 1 or args.orbit_adaptive != -1 or args.orbit_shutter != 1:
        print("--orbit-samples, --orbit-adaptive and --orbit-shutter go with --orbit K", file=sys.stderr)
        return 1
    if args.lens:
        if args.lens < 0 or not (args.focus > 0 or args.focus_at) or args.adaptive != -1 or args.frames != 1 or args.pick:
            print("--lens R takes a radius > 0 and --focus D > 0 (or --focus-at X,Y); not with --adaptive, --frames or --pick", file=sys.stderr)
            return 1
        return lens(sc, args, w, h)
    r = gpu.Renderer(args.device)
    r.set_samples(args.samples)          # before prepare(): the scene's own kernel then carries the supersampling form
    if args.adaptive != -1:
        r.set_adaptive_samples(args.adaptive)
    if args.pick:
        r.set_ray_queries(True)          # ... and the query kernel
    r.prepare(sc, wait=not args.pick or bool(args.out))      # (one ray does not wait for the scene compiler: the interpreter answers)
    if args.pick:
        x, y = pixel_arg(args.pick, w, h)
        print(pick_line(x, y, r.pick(x, y, w, h, args.max_steps)))
        if not args.out:
            r.close()
            return 0
    surf = np.zeros((h, w), dtype=np.uint32)
    for f in range(args.frames):
        t0 = time.perf_counter()
        r.render_host(surf.ctypes.data, w, h, args.max_steps)
        dt = (time.perf_counter() - t0) * 1e3
        print(f"Frame {f + 1}: {dt:.3f}ms  {w * h / dt / 1e3:.1f} Mpixels/s  [{r.kernel_name()}]")
    if args.out:
        write_ppm(args.out, surf)
    r.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
