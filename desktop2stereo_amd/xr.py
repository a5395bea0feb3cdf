"""The OpenXR viewer's screen and eye images for ops.dibr_xr_eyes / Engine.view_pipeline_xr (include/d2s.h d2s_xr_screen, d2s_xr_eye).

XrScreen is the screen in world space; its host helpers restate the reference's geometry for callers and for the tests --
model_mat4 = _build_model_mat4 (xr_viewer/screen.py:29-70), curved_verts = _build_curved_screen_verts (screen.py:110-173),
basis = _screen_effect_basis (xr_viewer/effects.py:65-82), fov_to_proj_mat4 / pose_to_view_mat4 = _fov_to_proj_mat4 /
_pose_to_view_mat4 (xr_viewer/render.py:981-1041) -- in float64 (the reference rounds each to float32).  The library does not call
them: it forms the surface itself, in double precision, from the struct.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

from . import _lib

CURVED_HALF_ANGLE_RAD = 0.6 * 0.8          # xr_viewer/constants.py:50-51
CURVED_SEGMENTS = 48                       # effects.py:1116


@dataclass
class XrScreen:
    """The reference's screen_* state.  curve: "flat" | "horizontal" | "vertical"; sizes in metres, angles in radians; roll is also
    the shader's u_roll; clear: the background (r, g, b in 0..1, a)."""
    width: float = 2.4
    height: float = 1.35
    distance: float = 2.0
    pan_x: float = 0.0
    pan_y: float = 0.0
    yaw: float = 0.0
    pitch: float = 0.0
    roll: float = 0.0
    curve: str = "flat"
    normal_offset: float = 0.0
    clear: Tuple[float, float, float, float] = (0.0, 0.0, 0.0, 1.0)

    def c_struct(self) -> "_lib.XrScreen":
        if self.curve not in _lib.XR_CURVE:
            raise ValueError(f"curve must be one of {list(_lib.XR_CURVE)}")
        if len(self.clear) != 4:
            raise ValueError("clear must be (r, g, b, a)")
        return _lib.XrScreen(C.sizeof(_lib.XrScreen), _lib.XR_CURVE[self.curve], float(self.width), float(self.height),
                             float(self.distance), float(self.pan_x), float(self.pan_y), float(self.yaw), float(self.pitch),
                             float(self.roll), float(self.normal_offset), (C.c_float * 4)(*[float(v) for v in self.clear]))

    def basis(self) -> Tuple[np.ndarray, np.ndarray]:
        """(R [4,4], centre [3]): the screen's rotation (yaw, pitch, roll) and its centre (pan_x, pan_y, -distance)."""
        cy, sy = math.cos(self.yaw), math.sin(self.yaw)
        cp, sp = math.cos(self.pitch), math.sin(self.pitch)
        cr, sr = math.cos(self.roll), math.sin(self.roll)
        R = np.array([[cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr, sy * cp, 0.0],
                      [cp * sr, cp * cr, -sp, 0.0],
                      [-sy * cr + cy * sp * sr, sy * sr + cy * sp * cr, cy * cp, 0.0],
                      [0.0, 0.0, 0.0, 1.0]])
        return R, np.array([self.pan_x, self.pan_y, -self.distance], np.float64)

    def model_mat4(self) -> np.ndarray:
        """T @ R @ S: the flat quad's corners are model @ (+-1, +-1, 0, 1)."""
        R, centre = self.basis()
        S = np.diag([self.width / 2.0, self.height / 2.0, 1.0, 1.0])
        T = np.eye(4)
        T[:3, 3] = centre + R[:3, 2] * self.normal_offset
        return T @ R @ S

    def curved_verts(self) -> np.ndarray:
        """[(48 + 1) * 2, 5] = x y z u v of the curved TRIANGLE_STRIP in world space (curve "flat" builds the horizontal arc, as the
        reference does)."""
        R, centre = self.basis()
        rot, n = R[:3, :3], CURVED_SEGMENTS + 1
        half_w, half_h = self.width / 2.0, self.height / 2.0
        angles = np.linspace(-CURVED_HALF_ANGLE_RAD, CURVED_HALF_ANGLE_RAD, n)
        ts = np.linspace(0.0, 1.0, n)
        vert = self.curve == "vertical"
        radius = (half_h if vert else half_w) / CURVED_HALF_ANGLE_RAD
        out = np.empty((n * 2, 5), np.float64)
        for i, (ang, t) in enumerate(zip(angles, ts)):
            along, lz = radius * math.sin(ang), radius * (1.0 - math.cos(ang))
            for j in range(2):
                local = np.array([(-half_w, half_w)[j], along, lz]) if vert else np.array([along, (-half_h, half_h)[j], lz])
                out[i * 2 + j, :3] = centre + rot @ local + rot[:, 2] * self.normal_offset
                out[i * 2 + j, 3:] = (float(j), t) if vert else (t, float(j))
        return out

    def _curved_frame(self):
        """(point(t, ac), direction(ang) * length, length, radius, a point of the cylinder's axis) of the arc: t = the strip coordinate
        0..1, ac = the coordinate across it 0..1; screen coordinates (u, v) = (t, ac) for a horizontal curve, (ac, t) for a vertical one."""
        R, centre = self.basis()
        rot, vert = R[:3, :3], self.curve == "vertical"
        length, wid = (self.height, self.width) if vert else (self.width, self.height)
        radius = length / 2.0 / CURVED_HALF_ANGLE_RAD

        def local(al, ac, lz):
            return rot @ (np.array([ac, al, lz]) if vert else np.array([al, ac, lz]))

        def point(t, ac):
            ang = -CURVED_HALF_ANGLE_RAD + 2.0 * CURVED_HALF_ANGLE_RAD * t
            return centre + local(radius * math.sin(ang), (ac - 0.5) * wid, radius * (1.0 - math.cos(ang)))
        return point, (lambda ang: local(math.cos(ang) * length, 0.0, math.sin(ang) * length)), length, radius, centre + local(0.0, 0.0, radius)

    def glow_pieces(self, glow: "XrGlow" = None) -> list:
        """The curved glow's band mesh (_build_curved_glow_band_verts, xr_viewer/effects.py:314-406) as the planar pieces the library
        draws: [(name, p00, p10, p01, g00, g10, g01)] -- three corners in world space and the screen coordinates (ga, gb) there, both
        affine over the piece.  "facet<i>": the strip's facets, unbounded across the strip; "tangent0" / "tangent1": the tangent planes
        at the arc's ends (p10 = one screen length along the tangent); with a glow: "chord0" / "chord1", the inner band's planes at
        the ends, from the end to the strip coordinate inner_uv / inner_(w | h) (the mesh has them for "glow2" too, which never draws
        its inner vertices)."""
        if self.curve == "flat":
            raise ValueError("glow_pieces: the screen is flat")
        point, tangent, _, _, _ = self._curved_frame()
        vert = self.curve == "vertical"
        g = (lambda t, ac: (ac, t)) if vert else (lambda t, ac: (t, ac))
        n = CURVED_SEGMENTS
        ts = [i / n for i in range(n + 1)]
        out = [(f"facet{i}", point(ts[i], 0.0), point(ts[i + 1], 0.0), point(ts[i], 1.0), g(ts[i], 0.0), g(ts[i + 1], 0.0), g(ts[i], 1.0))
               for i in range(n)]
        for k, ang in enumerate((-CURVED_HALF_ANGLE_RAD, CURVED_HALF_ANGLE_RAD)):
            p = point(float(k), 0.0)
            out.append((f"tangent{k}", p, p + tangent(ang), point(float(k), 1.0), g(float(k), 0.0), g(k + 1.0, 0.0), g(float(k), 1.0)))
        if glow is not None and glow.mode != "off":
            u = glow.uniforms(self)
            inner_uv = min(u["inner_w"], u["inner_h"]) * max(float(glow.inner_edge_fraction), 0.0)
            e = min(0.5, inner_uv / (u["inner_h"] if vert else u["inner_w"]))
            for k, (t0, t1) in enumerate(((0.0, e), (1.0 - e, 1.0))):
                out.append((f"chord{k}", point(t0, 0.0), point(t1, 0.0), point(t0, 1.0), g(t0, 0.0), g(t1, 0.0), g(t0, 1.0)))
        return out

    def eye_inside(self, vp) -> bool:
        """Whether the eye of vp = proj @ view (its position: the null space of vp's x, y and w rows) lies inside the convex region the
        curved screen and its two tangent planes bound, by 1e-4 of the arc's radius: what d2s_dibr_xr_eyes_glow_curved demands of every
        eye (outside it the glow's translucent pieces overlap).  True for a flat screen."""
        if self.curve == "flat":
            return True
        m = np.array(vp, np.float64).reshape(4, 4)[[0, 1, 3]]
        h = np.array([(-1.0) ** k * np.linalg.det(np.delete(m, k, axis=1)) for k in range(4)])
        if not abs(h[3]) > 1e-12 * np.abs(h[:3]).max() or not abs(h[3]) > 0.0:
            return False
        eye = h[:3] / h[3]
        _, _, _, radius, axis = self._curved_frame()
        for _, p00, p10, p01, *_ in self.glow_pieces():
            nrm = np.cross(p10 - p00, p01 - p00)
            de, da = float(nrm @ (eye - p00)), float(nrm @ (axis - p00))
            if not (-de if da < 0 else de) > 1e-4 * radius * float(np.linalg.norm(nrm)):
                return False
        return True


@dataclass
class XrGlow:
    """The reference's glow around the flat screen (include/d2s.h d2s_xr_glow): mode "glow" | "glow2" | "off"; range_m: what
    _glow_range_m returns (glow_range_m below; the library halves it for glow2, as _render_glow does); inner_edge_fraction:
    _glow_inner_edge_fraction, the inner band's width as a share of the screen's shorter side in glow uv."""
    mode: str = "glow"
    range_m: float = 15.0
    inner_edge_fraction: float = 0.075

    def c_struct(self) -> "_lib.XrGlow":
        if self.mode not in _lib.XR_GLOW:
            raise ValueError(f"glow mode must be one of {list(_lib.XR_GLOW)}")
        return _lib.XrGlow(C.sizeof(_lib.XrGlow), _lib.XR_GLOW[self.mode], float(self.range_m), float(self.inner_edge_fraction))

    def uniforms(self, screen: "XrScreen") -> dict:
        """What _render_glow (xr_viewer/effects.py:486-495, 575-580) hands its shader for this screen, in float64: glow_w, glow_h,
        inner_w, inner_h, u_screen_half, u_glow_inv_range, u_glow_inner.  The library forms the same numbers itself."""
        rng = max(float(self.range_m), 1e-4) * (0.5 if self.mode == "glow2" else 1.0)
        glow_w, glow_h = screen.width + 2 * rng, screen.height + 2 * rng
        inner_w, inner_h = screen.width / glow_w, screen.height / glow_h
        inner_uv = 0.0 if self.mode == "glow2" else min(inner_w, inner_h) * max(float(self.inner_edge_fraction), 0.0)
        return dict(glow_w=glow_w, glow_h=glow_h, inner_w=inner_w, inner_h=inner_h, u_screen_half=(inner_w * 0.5, inner_h * 0.5),
                    u_glow_inv_range=1.0 / max(rng / max(glow_w, glow_h), 1e-6), u_glow_inner=inner_uv)


FROST_GRID = 8                             # _FLAT_FROST_N = _FLAT_FROST_M (effects.py:140-141)


@dataclass
class XrFrost:
    """The reference's "veil" and "frosted" looks around the flat screen (include/d2s.h d2s_xr_frost): four translucent walls from the
    screen's edges towards the viewer, blended over the eye image after the screen.  mode "veil" | "frosted" | "off"; head: the head
    position in world space; intensity: ALREADY multiplied by max(_glow_intensity_multiplier, 0).  The other fields are the uniforms of
    _set_frost_veil_uniforms / _set_frost_uniform_values (xr_viewer/effects.py:651-718); veil() and frosted() carry the reference's
    defaults (xr_viewer/implementation.py:354-366).  The host helpers restate the reference's geometry in float64 for callers and
    tests; the library forms the same numbers itself from the struct."""
    mode: str = "veil"
    head: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    intensity: float = 1.5
    alpha: float = 1.0
    edge_inset: float = 0.02
    beam_softness: float = 0.34
    beam_thickness: float = 3.0
    lod: float = 5.4
    threshold: float = 0.46
    noise_scale: float = 54.0
    blend: float = 1.35
    diffuse: float = 0.85
    time: float = 0.0

    @classmethod
    def veil(cls, head=(0.0, 0.0, 0.0), multiplier: float = 1.0, **kw) -> "XrFrost":
        """_render_frost_veil's defaults: intensity 1.5 * multiplier, alpha 1, inset 0.02, softness 0.34, thickness 3."""
        return cls(**{**dict(mode="veil", head=tuple(head), intensity=1.5 * max(float(multiplier), 0.0)), **kw})

    @classmethod
    def frosted(cls, head=(0.0, 0.0, 0.0), multiplier: float = 1.0, time: float = 0.0, **kw) -> "XrFrost":
        """_render_frost_glow's defaults: intensity 1 * multiplier, alpha 0.42, inset 0.045, thickness 1.6, LOD 5.4, threshold 0.46,
        noise scale 54, blend 1.35, diffuse 0.85."""
        return cls(**{**dict(mode="frosted", head=tuple(head), intensity=1.0 * max(float(multiplier), 0.0), alpha=0.42, edge_inset=0.045,
                             beam_thickness=1.6, time=float(time)), **kw})

    def c_struct(self) -> "_lib.XrFrost":
        if self.mode not in _lib.XR_FROST:
            raise ValueError(f"frost mode must be one of {list(_lib.XR_FROST)}")
        if len(self.head) != 3:
            raise ValueError("head must be (x, y, z)")
        return _lib.XrFrost(C.sizeof(_lib.XrFrost), _lib.XR_FROST[self.mode], (C.c_double * 3)(*[float(v) for v in self.head]),
                            float(self.intensity), float(self.alpha), float(self.edge_inset), float(self.beam_softness),
                            float(self.beam_thickness), float(self.lod), float(self.threshold), float(self.noise_scale), float(self.blend),
                            float(self.diffuse), float(self.time))

    def draws(self) -> bool:
        """Whether the walls are drawn at all (the reference's early returns, effects.py:822-857): otherwise the call is dibr_xr_eyes."""
        return self.mode != "off" and self.intensity > 0.0 and not (self.mode == "veil" and self.alpha <= 0.002)

    def layout(self, screen: "XrScreen") -> Tuple[float, float, float]:
        """(front_depth, front_half_w, front_half_h) of _frost_front_layout (effects.py:120-128), without its rounded cache key."""
        R, centre = screen.basis()
        hl = R[:3, :3].T @ (np.asarray(self.head, np.float64) - centre)
        return (max(float(hl[2]) + 0.55, float(screen.distance) + 0.35, 0.75),
                max(float(screen.width) * 0.5, abs(float(hl[0])) + 0.65, 0.65),
                max(float(screen.height) * 0.5, abs(float(hl[1])) + 0.65, 0.65))

    def model_mat4(self, screen: "XrScreen") -> np.ndarray:
        """_screen_effect_model(width, height, z_scale=front_depth): the walls' local frame -> world."""
        R, centre = screen.basis()
        T = np.eye(4)
        T[:3, 3] = centre
        return T @ R @ np.diag([screen.width / 2.0, screen.height / 2.0, self.layout(screen)[0], 1.0])

    def wall_verts(self, screen: "XrScreen") -> np.ndarray:
        """[4, 158, 5] = x y t u v: the four TRIANGLE_STRIPs of _build_flat_frost_verts (effects.py:145-187) in draw order top, bottom,
        left, right, in the walls' local frame -- 8 depth rows of 2 * 9 vertices, stitched with 2 degenerate vertices each."""
        _, fhw, fhh = self.layout(screen)
        fx, fy = fhw / max(screen.width * 0.5, 1e-6), fhh / max(screen.height * 0.5, 1e-6)
        n = FROST_GRID
        out = []
        for (ax, ay, uva, bx, by, uvb) in ((-1, 1, (0, 0), 1, 1, (1, 0)), (-1, -1, (0, 1), 1, -1, (1, 1)), (-1, 1, (0, 0), -1, -1, (0, 1)),
                                           (1, 1, (1, 0), 1, -1, (1, 1))):
            def vtx(s, t):
                px, py = ax + s * (bx - ax), ay + s * (by - ay)
                return [px + t * (px * fx - px), py + t * (py * fy - py), t, uva[0] + s * (uvb[0] - uva[0]), uva[1] + s * (uvb[1] - uva[1])]
            wall, prev_last = [], None
            for i in range(n):
                row = []
                for j in range(n + 1):
                    row += [vtx(j / n, i / n), vtx(j / n, (i + 1) / n)]
                if prev_last is not None:
                    wall += [prev_last, row[0]]
                wall += row
                prev_last = row[-1]
            out.append(wall)
        return np.array(out, np.float64)

    def curved_wall_verts(self, screen: "XrScreen") -> np.ndarray:
        """[588, 8] = world x y z, v_uv = (u, 1 - v), v_local = (2u - 1, 2v - 1, t): the one TRIANGLES draw of
        _build_curved_frost_verts (effects.py:189-254) around a curved screen, in float64 -- 98 quads (rear0, rear1, front0), (front0,
        rear1, front1): two long walls of 48 quads along the arc's curved edges (horizontal: the top edge, then the bottom; vertical:
        u = 0, then u = 1), then one quad at each end of the arc.  rear: a strip vertex (t = 0, uv as the strip stores it, float32);
        front: centre + R @ ((2u - 1) * front_half_w, (2v - 1) * front_half_h, front_depth) (t = 1).  The library
        (d2s_dibr_xr_eyes_frost_curved) draws these 196 triangles."""
        if screen.curve == "flat":
            raise ValueError("curved_wall_verts: the screen is flat")
        fd, fhw, fhh = self.layout(screen)
        R, centre = screen.basis()
        strip = screen.curved_verts()
        strip[:, 3:] = strip[:, 3:].astype(np.float32)
        n = CURVED_SEGMENTS

        def pair(col, side):
            x, y, z, u, v = strip[col * 2 + side]
            f = centre + R[:3, :3] @ np.array([(u * 2.0 - 1.0) * fhw, (v * 2.0 - 1.0) * fhh, fd])
            attr = [u, 1.0 - v, u * 2.0 - 1.0, v * 2.0 - 1.0]
            return [x, y, z, *attr, 0.0], [f[0], f[1], f[2], *attr, 1.0]

        out = []

        def quad(a, b):
            (r0, f0), (r1, f1) = a, b
            out.extend([r0, r1, f0, f0, r1, f1])
        for side in ((0, 1) if screen.curve == "vertical" else (1, 0)):
            for i in range(n):
                quad(pair(i, side), pair(i + 1, side))
        for col in (0, n):
            quad(pair(col, 0), pair(col, 1))
        return np.array(out, np.float64)

    def uniforms(self, screen: "XrScreen" = None, crop=(0.0, 0.0, 1.0, 1.0)) -> dict:
        """What the mode's setter hands its program (effects.py:651-718): the veil's five, frosted's eleven, and u_source_crop."""
        u = dict(u_source_crop=tuple(float(v) for v in crop), u_edge_inset=float(self.edge_inset), u_intensity=float(self.intensity),
                 u_frost_alpha=float(self.alpha), u_beam_softness=float(self.beam_softness), u_beam_thickness=float(self.beam_thickness))
        if self.mode == "frosted":
            u.update(u_lod=float(self.lod), u_threshold=float(self.threshold), u_noise_scale=float(self.noise_scale),
                     u_frost_blend=float(self.blend), u_diffuse_scatter=float(self.diffuse), u_time=float(self.time))
        return u


def _rot_yx(yaw: float, pitch: float) -> np.ndarray:
    """rot_y(yaw) @ rot_x(pitch) [4,4]: the rotation the reference gives its panels (no roll; overlay.py:210-219, 1363-1372)."""
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    return (np.array([[cy, 0.0, sy, 0.0], [0.0, 1.0, 0.0, 0.0], [-sy, 0.0, cy, 0.0], [0.0, 0.0, 0.0, 1.0]]) @
            np.array([[1.0, 0.0, 0.0, 0.0], [0.0, cp, -sp, 0.0], [0.0, sp, cp, 0.0], [0.0, 0.0, 0.0, 1.0]]))


@dataclass
class XrPanel:
    """One world-space panel of the eye image (include/d2s.h d2s_xr_panel; ops.dibr_xr_panels): the unit quad (+-1, +-1, 0, 1) under
    the affine `model` [4,4], as the reference draws its status panel, OSDs, keyboard, key highlights and laser quads after the
    screen.  texture: an index into the call's textures (the reference's _OVERLAY_FRAG: the picture at uv, alpha times `alpha`), or
    None: the solid `color` (r, g, b in 0..1, a; _SOLID_FRAG).  depth_test: GL_LESS against the screen and the earlier panels that
    wrote depth; depth_write (acts only with depth_test, as in GL); blend: SRC_ALPHA, ONE_MINUS_SRC_ALPHA, alpha included.  The
    constructors restate the reference's placements in float64 (the reference rounds each matrix to float32)."""
    model: np.ndarray
    texture: int = None
    color: Tuple[float, float, float, float] = (1.0, 1.0, 1.0, 1.0)
    alpha: float = 1.0
    depth_test: bool = True
    depth_write: bool = True
    blend: bool = True

    def c_struct(self) -> "_lib.XrPanel":
        m = np.asarray(self.model, np.float64)
        if m.shape != (4, 4):
            raise ValueError("XrPanel.model must be [4,4]")
        if len(self.color) != 4:
            raise ValueError("XrPanel.color must be (r, g, b, a)")
        flags = (_lib.XR_PANEL_DEPTH_TEST if self.depth_test else 0) | (_lib.XR_PANEL_DEPTH_WRITE if self.depth_write else 0) | \
            (_lib.XR_PANEL_BLEND if self.blend else 0)
        return _lib.XrPanel((C.c_double * 16)(*m.ravel()), -1 if self.texture is None else int(self.texture), flags,
                            (C.c_float * 4)(*[float(v) for v in self.color]), float(self.alpha), C.sizeof(_lib.XrPanel))

    @classmethod
    def below_screen(cls, screen: "XrScreen", tex_size, texture: int = 0, alpha: float = 1.0) -> "XrPanel":
        """The FPS / status panel's placement (_render_fps_overlay, xr_viewer/overlay.py:194-229): T @ R @ T_local @ S -- in the
        screen's plane (yaw and pitch; the reference leaves the roll out), below its bottom edge by 2 % of the screen's height,
        left-aligned, an eighth of the screen's height tall and tex_size = (width, height)'s aspect wide.  alpha: u_alpha (the
        reference fades it to 0.15 while a trigger is held on it).  Blended, depth-tested, writes depth."""
        ow, oh = tex_size
        sh, sx, sy = float(screen.height), screen.width / 2.0, screen.height / 2.0
        h = sh / 8.0
        w = h * (float(ow) / float(oh))
        T, Tl = np.eye(4), np.eye(4)
        T[:3, 3] = (screen.pan_x, screen.pan_y, -screen.distance)
        Tl[0, 3], Tl[1, 3] = -sx + w / 2.0, -sy - sh * 0.02 - h / 2.0
        return cls(T @ _rot_yx(screen.yaw, screen.pitch) @ Tl @ np.diag([w / 2.0, h / 2.0, 1.0, 1.0]), texture=texture, alpha=alpha)

    @staticmethod
    def keyboard_world(pan_x: float, pan_y: float, distance: float, yaw: float, pitch: float) -> np.ndarray:
        """_kb_world_mat (xr_viewer/overlay.py:1356-1379): translate(pan_x, pan_y, -distance) @ rot_y(yaw) @ rot_x(pitch)."""
        T = np.eye(4)
        T[:3, 3] = (pan_x, pan_y, -distance)
        return T @ _rot_yx(yaw, pitch)

    @classmethod
    def keyboard_group(cls, kb_world, width: float, height: float, border_alpha: float = 0.0, highlights=(), texture: int = 0) -> list:
        """The keyboard's draws in order (_render_keyboard, xr_viewer/overlay.py:1427-1510), all blended and depth-tested, none writing
        depth: with border_alpha > 0 the solid border (0.3, 0.7, 1.0, border_alpha), 8 mm larger each way and 1 mm behind the
        surface; the keyboard, `texture` over width x height metres; then one solid quad 1 mm in front per highlight =
        ((x0, y0, x1, y1) in metres in the keyboard's frame, (r, g, b, a))."""
        kb = np.asarray(kb_world, np.float64).reshape(4, 4)
        kw2, kh2 = width / 2.0, height / 2.0
        flags = dict(depth_test=True, depth_write=False, blend=True)
        out = []
        if border_alpha > 0.0:
            m = np.diag([kw2 + 0.008, kh2 + 0.008, 1.0, 1.0])
            m[2, 3] = -0.001
            out.append(cls(kb @ m, color=(0.3, 0.7, 1.0, float(border_alpha)), **flags))
        out.append(cls(kb @ np.diag([kw2, kh2, 1.0, 1.0]), texture=texture, **flags))
        for (x0, y0, x1, y1), color in highlights:
            m = np.diag([(x1 - x0) / 2.0, (y1 - y0) / 2.0, 1.0, 1.0])
            m[:3, 3] = ((x0 + x1) / 2.0, (y0 + y1) / 2.0, 0.001)
            out.append(cls(kb @ m, color=tuple(float(v) for v in color), **flags))
        return out


def glow_range_m(screen: XrScreen, head=None, width_m: float = 0.75, ref_screen: float = 2.4) -> float:
    """_glow_range_m (xr_viewer/effects.py:280-312) without its rounded-key cache: the glow's reach in metres, growing with the
    screen's longer side (rounded to centimetres, as the reference's key rounds it) and with the head's distance from the screen's
    centre (head = the head position in world space, None = the origin)."""
    base_width = max(float(width_m or 0.75), 0.75)
    ref = max(float(ref_screen or 2.4), 1e-6)
    screen_long = max(round(float(screen.width), 2), round(float(screen.height), 2), ref)
    sd = round(float(screen.distance or 2.0), 1)
    hx, hy, hz = (0.0, 0.0, 0.0) if head is None else (float(v) for v in head)
    dx, dy, dz = hx - float(screen.pan_x), hy - float(screen.pan_y), hz + sd
    dist = max(math.sqrt(dx * dx + dy * dy + dz * dz), 0.5)
    return base_width * (screen_long / ref) * (dist / 2.0) * 20.0


def fov_to_proj_mat4(angle_left: float, angle_right: float, angle_up: float, angle_down: float, near: float = 0.05,
                     far: float = 100.0) -> np.ndarray:
    """XrFovf -> the OpenGL asymmetric-frustum projection (numpy's row / column convention)."""
    l, r = math.tan(angle_left) * near, math.tan(angle_right) * near
    t, b = math.tan(angle_up) * near, math.tan(angle_down) * near
    if abs(r - l) < 1e-6:
        r += 1e-6
    if abs(t - b) < 1e-6:
        t += 1e-6
    p = np.zeros((4, 4))
    p[0, 0], p[0, 2] = 2 * near / (r - l), (r + l) / (r - l)
    p[1, 1], p[1, 2] = 2 * near / (t - b), (t + b) / (t - b)
    p[2, 2], p[2, 3] = -(far + near) / (far - near), -2 * far * near / (far - near)
    p[3, 2] = -1.0
    return p


def pose_to_view_mat4(orientation: Sequence[float], position: Sequence[float]) -> np.ndarray:
    """XrPosef (orientation = quaternion x, y, z, w; position) -> the view matrix (the pose's inverse)."""
    x, y, z, w = (float(v) for v in orientation)
    tx, ty, tz = (float(v) for v in position)
    r00, r01, r02 = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    r10, r11, r12 = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    r20, r21, r22 = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return np.array([[r00, r10, r20, -(r00 * tx + r10 * ty + r20 * tz)],
                     [r01, r11, r21, -(r01 * tx + r11 * ty + r21 * tz)],
                     [r02, r12, r22, -(r02 * tx + r12 * ty + r22 * tz)],
                     [0.0, 0.0, 0.0, 1.0]])


def xr_eye(vp, width: int, height: int, eye: int, flip_y: bool = False) -> "_lib.XrEye":
    """One swapchain image: vp = proj @ view [4,4], its size, eye 0 (left) | 1 (right).  flip_y: negate proj's row 1 -- which is row 1
    of proj @ view -- as the reference's _render_eye(flip_y=True) does (the library leaves it to the caller)."""
    m = np.array(vp, np.float64).reshape(4, 4)
    if flip_y:
        m[1, :] = -m[1, :]
    return _lib.XrEye((C.c_double * 16)(*m.ravel()), int(width), int(height), int(eye), C.sizeof(_lib.XrEye))


def eye_array(eyes) -> "C.Array":
    """A sequence of 1 or 2 xr_eye structs (or (vp, width, height, eye) tuples) as the C array the library takes."""
    es = [e if isinstance(e, _lib.XrEye) else xr_eye(*e) for e in eyes]
    if len(es) not in (1, 2):
        raise ValueError("eyes must name 1 or 2 eye images")
    return (_lib.XrEye * len(es))(*es)


def panorama_rays(proj, view) -> np.ndarray:
    """[3,3] float64, NDC (x, y, 1) -> the un-normalised world direction of that pixel's ray, as _render_panorama_background and
    _PANORAMA_FRAG form it (xr_viewer/effects.py:992-1015, xr_viewer/glsl.py:81-83): view's rotation transposed times inv(proj)
    applied to (x, y, 1, 1).  The shader's division by max(|w|, 1e-6) and its two normalisations scale by a positive number, which the
    direction's angles do not see.  proj is passed in already y-flipped when the eye is, as _render_eye does."""
    a = np.linalg.inv(np.array(proj, np.float64).reshape(4, 4))
    n = np.stack([a[:3, 0], a[:3, 1], a[:3, 2] + a[:3, 3]], 1)
    return np.array(view, np.float64).reshape(4, 4)[:3, :3].T @ n


@dataclass
class XrPanorama:
    """The reference's panorama background (include/d2s.h d2s_xr_panorama): _panorama_background_settings' yaw_offset_deg, exposure
    and flip_y (xr_viewer/effects.py:981-990).  The image itself (uint8 [height, width, 3], row 0 up) and its mip_chain travel beside
    it as tensors.  Drawn behind every look: ops.dibr_xr_eyes_panorama (plain, and the flat screen's glow, veil and frosted) and
    ops.dibr_xr_eyes_panorama_curved (those, and the curved screen's)."""
    yaw_offset_deg: float = 0.0
    exposure: float = 1.0
    flip_y: bool = False

    def c_struct(self, eyes_proj_view, image_shape) -> "_lib.XrPanorama":
        """eyes_proj_view: one (proj, view) pair per eye image, in the order of eyes[] (proj y-flipped where the eye is);
        image_shape: the panorama's (height, width)."""
        pv = list(eyes_proj_view)
        if len(pv) not in (1, 2):
            raise ValueError("eyes_proj_view must name 1 or 2 (proj, view) pairs")
        s = _lib.XrPanorama()
        s.struct_size = C.sizeof(_lib.XrPanorama)
        s.flip_y = 1 if self.flip_y else 0
        s.height, s.width = int(image_shape[0]), int(image_shape[1])
        s.yaw_offset = float(self.yaw_offset_deg) / 360.0
        s.exposure = float(self.exposure)
        for i, (proj, view) in enumerate(pv):
            for k, v in enumerate(panorama_rays(proj, view).ravel()):
                s.ray[i][k] = float(v)
        return s
