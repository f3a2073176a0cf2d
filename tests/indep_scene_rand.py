"""The visual randomisation's draw, restated (test infrastructure; numpy only).

Nothing here is shared with csrc/: Philox4x32-10 is written out from its definition (Salmon et al., "Parallel random numbers: as easy
as 1, 2, 3", SC'11; the multipliers and Weyl constants of Random123's philox.h) with Python integers, and the rule of mcg_scene_randomize
(include/mcg.h) from its description: which draw feeds which quantity, and how a uniform becomes a value.

Keying: counter = (global id low word, episode, draw index, stream ^ (global id high word << 8)), key = (seed low, seed high); the
stream of the pictures is 2.  A draw yields the pair (u0, u1): the two 64-bit halves of the output, top 53 bits each, times 2^-53.
A mapped value is lo + (hi - lo) * u.  There is no fused multiply-add here, so a value may differ from the kernel's in its last bit.
A zero offset, a zero tilt and a zero rotation vector leave the base's values as they are, signed zeros included: with all half ranges
zero and all scales (1, 1) a row is the base row bit for bit.

A row (40 doubles): cam_pos 0-2, cam_mat 3-11 (row-major), fovy 12, light_dir 13-15, light ambient / diffuse 16 / 17, headlight
ambient / diffuse 18 / 19, the colours of ground, table, cube, target, mesh, sky 20-37, two zeros.
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STREAM = 2
WORLD_DRAWS, CAM_BASE, CAM_DRAWS = 12, 32, 4
RANGE_KEYS = ("cam_pos", "cam_rot", "fovy_scale", "light_tilt", "light_ambient_scale", "light_diffuse_scale", "head_scale", "rgb")


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = (int(x) & MASK for x in ctr)
    k0, k1 = (int(x) & MASK for x in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [c0, c1, c2, c3]


def pair(seed: int, gid: int, episode: int, draw: int, stream: int = STREAM):
    seed &= 2 ** 64 - 1
    gid &= 2 ** 64 - 1
    r = philox4x32_10([gid & MASK, episode & MASK, draw, stream ^ (((gid >> 32) & MASK) << 8) & MASK], [seed & MASK, seed >> 32])
    return (((r[0] << 32) | r[1]) >> 11) * 2.0 ** -53, (((r[2] << 32) | r[3]) >> 11) * 2.0 ** -53


def _ranges(ranges: dict) -> dict:
    """Every field, with the "no jitter" value where a key is missing; rgb: one number, six, or a dict by class."""
    assert set(ranges) <= set(RANGE_KEYS), sorted(set(ranges) - set(RANGE_KEYS))
    out = {"cam_pos": np.broadcast_to(np.asarray(ranges.get("cam_pos", 0.0), dtype=np.float64), (3,)),
           "cam_rot": np.broadcast_to(np.asarray(ranges.get("cam_rot", 0.0), dtype=np.float64), (3,)),
           "light_tilt": float(ranges.get("light_tilt", 0.0))}
    for k in ("fovy_scale", "light_ambient_scale", "light_diffuse_scale", "head_scale"):
        out[k] = tuple(float(x) for x in ranges.get(k, (1.0, 1.0)))
    rgb = ranges.get("rgb", 0.0)
    if isinstance(rgb, dict):
        rgb = [rgb.get(k, 0.0) for k in ("ground", "table", "cube", "target", "mesh", "sky")]
    out["rgb"] = np.broadcast_to(np.asarray(rgb, dtype=np.float64), (6,))
    return out


def _lerp(lo, hi, u):
    return lo + (hi - lo) * u


def _add(x, d):
    """x + d; a zero offset leaves x as it is, a signed zero included (as a zero tilt and a zero rotation vector do)."""
    return x if d == 0.0 else x + d


def rotation(w):
    """R(w) = I + a K + b K^2, K = [w]x, a = sin|w| / |w|, b = (1 - cos|w|) / |w|^2 (a = 1, b = 1/2 below |w| = 1e-12)."""
    w = np.asarray(w, dtype=np.float64)
    th = float(np.sqrt(w @ w))
    a, b = (1.0, 0.5) if th < 1e-12 else (np.sin(th) / th, (1.0 - np.cos(th)) / (th * th))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + a * K + b * (K @ K)


def row(base_row, ranges: dict, seed: int, gid: int, episode: int, cam_slot: int = 0) -> np.ndarray:
    """The row of the environment with global id ``gid`` in its episode ``episode``, from the base scene's row."""
    assert 0 <= cam_slot < 8
    base = np.asarray(base_row, dtype=np.float64)
    R = _ranges(ranges)
    out = np.zeros(40)
    U = lambda draw: pair(seed, gid, episode, draw)
    # the world block: light and colours, the same for every camera of the environment
    u0, u1 = U(0)
    theta, phi = R["light_tilt"] * np.sqrt(u0), 2.0 * np.pi * u1
    d0 = base[13:16]
    e1 = np.cross([0.0, 1.0, 0.0] if abs(d0[0]) > 0.9 else [1.0, 0.0, 0.0], d0)
    e1 = e1 / np.sqrt(e1 @ e1)
    e2 = np.cross(d0, e1)
    out[13:16] = d0 if theta == 0.0 else np.cos(theta) * d0 + np.sin(theta) * (np.cos(phi) * e1 + np.sin(phi) * e2)
    u0, u1 = U(1)
    out[16] = base[16] * _lerp(*R["light_ambient_scale"], u0)
    out[17] = base[17] * _lerp(*R["light_diffuse_scale"], u1)
    u0, _ = U(2)
    s = _lerp(*R["head_scale"], u0)
    out[18], out[19] = base[18] * s, base[19] * s
    for k in range(9):
        us = U(3 + k)
        for j in range(2):
            ch = 2 * k + j
            h = R["rgb"][ch // 3]
            c = _add(base[20 + ch], _lerp(-h, h, us[j]))
            out[20 + ch] = 0.0 if c < 0.0 else (1.0 if c > 1.0 else c)
    # the camera block of this slot
    c = CAM_BASE + CAM_DRAWS * cam_slot
    (ux, uy), (uz, uf), (wx, wy), (wz, _) = U(c), U(c + 1), U(c + 2), U(c + 3)
    hp, hr = R["cam_pos"], R["cam_rot"]
    out[0:3] = [_add(base[k], _lerp(-hp[k], hp[k], u)) for k, u in enumerate((ux, uy, uz))]
    w = np.array([_lerp(-hr[0], hr[0], wx), _lerp(-hr[1], hr[1], wy), _lerp(-hr[2], hr[2], wz)])
    out[3:12] = base[3:12] if not w.any() else (rotation(w) @ base[3:12].reshape(3, 3)).reshape(-1)
    out[12] = base[12] * _lerp(*R["fovy_scale"], uf)
    return out


def table(base_row, ranges: dict, seed: int, gids, episodes, cam_slot: int = 0) -> np.ndarray:
    """[N, 40]: ``row`` for each (global id, episode)."""
    return np.stack([row(base_row, ranges, seed, int(g), int(e), cam_slot) for g, e in zip(gids, episodes)])
