"""The wall loads of ns_loads_* -- the scheme's own boundary fluxes per boundary face and their sums per edge -- stated
in NumPy ("Wall loads").  This file is the normative statement; the GPU kernels (k_load_faces,
k_load_edges) are tested against it, and it against the oracle (tests/test_loads_ref.py).  TEST INFRASTRUCTURE ONLY.

Built on derived_ref.DGrid (cells, face tags, velocity ghosts, the pressure's Laplacian) and scalar_ref's ghost
convention.  A boundary face is face k (0 W, 1 E, 2 S, 3 N) of a domain cell (i, j) whose neighbour there is not in
the domain; it belongs to the grid edge e = tag[i, j, k].  For a face

  n  = (DI[k], DJ[k]);  h = hx[i] for k < 2, hy[j] otherwise;  ds = the other spacing
  s  = the face centre's coordinate along the edge from the box's lower-left corner: 0.5 (yf[j] + yf[j + 1]) for
       k < 2, 0.5 (xf[i] + xf[i + 1]) otherwise, xf / yf the cumulative sums of hx / hy

  p  = derived_ref's P of the adjacent cell, phi - dt / (2 re) L phi, on every face type
  tx = (ghost_v(u, i, j, k, 0) - u) / (re h),  ty = (ghost_v(v, i, j, k, 1) - v) / (re h)
  un = face(u) n_x + face(v) n_y with Div_V's boundary-face values 0.5 (q + ghost)
  tb = 0.5 (T + ghostT),  qn = -(ghostT - T) / (pe h);  ghostT = T on a zero-gradient edge, -T + 2 value on a
       Dirichlet one; both exactly 0 without a scalar

Per edge, over its faces in ascending s (SUMS):
  len = sum ds   fpx = sum p n_x ds   fpy = sum p n_y ds   fvx = -sum tx ds   fvy = -sum ty ds
  q = sum un ds   heat = sum qn ds   heat_adv = sum un tb ds
The sums here are exactly rounded (math.fsum); any order of adding an edge's nf terms lies within
nf 2^-53 sum |term| of them."""
import math

import numpy as np

from derived_ref import DI, DJ

FACE_KEYS = ("s", "ds", "p", "tx", "ty", "un", "tb", "qn")
SUMS = ("len", "fpx", "fpy", "fvx", "fvy", "q", "heat", "heat_adv")


def face_list(G):
    """Per edge the boundary faces (i, j, k) in ascending s, with the arrays s and ds."""
    n_edges = len(G.bc)
    xf = np.concatenate([[0.0], np.cumsum(G.hx)])
    yf = np.concatenate([[0.0], np.cumsum(G.hy)])
    per = [[] for _ in range(n_edges)]
    for i, j in zip(*np.nonzero(G.mask)):
        for k in range(4):
            if G.inside(i + DI[k], j + DJ[k]):
                continue
            s = 0.5 * (yf[j] + yf[j + 1]) if k < 2 else 0.5 * (xf[i] + xf[i + 1])
            ds = G.hy[j] if k < 2 else G.hx[i]
            per[int(G.tag[i, j, k])].append((s, int(i), int(j), k, ds))
    out = []
    for faces in per:
        faces.sort()
        out.append({"cells": [(i, j, k) for _, i, j, k, _ in faces],
                    "s": np.array([f[0] for f in faces], dtype=np.float64),
                    "ds": np.array([f[4] for f in faces], dtype=np.float64)})
    return out


def face_values(G, dt, re, u, v, phi, scalar=None):
    """Per edge a dict of the FACE_KEYS arrays (and "cells").  scalar: (pe, T, sbc) with sbc[e] = ("dirichlet", value)
    or ("zerograd",) per edge; None: no scalar, tb = qn = 0."""
    alpha = dt / (2 * re)
    out = face_list(G)
    for e, F in enumerate(out):
        n = len(F["cells"])
        for key in FACE_KEYS[2:]:
            F[key] = np.zeros(n)
        for f, (i, j, k) in enumerate(F["cells"]):
            h = G.hx[i] if k < 2 else G.hy[j]
            nx, ny = float(DI[k]), float(DJ[k])
            F["p"][f] = phi[i, j] - alpha * G.lap(phi, i, j)
            F["tx"][f] = (G.ghost_v(u, i, j, k, 0) - u[i, j]) / (re * h)
            F["ty"][f] = (G.ghost_v(v, i, j, k, 1) - v[i, j]) / (re * h)
            F["un"][f] = G.face(u, i, j, k, 0) * nx + G.face(v, i, j, k, 1) * ny
            if scalar is not None:
                pe, T, sbc = scalar
                b = sbc[e]
                gT = T[i, j] if b[0] == "zerograd" else -T[i, j] + 2.0 * b[1]
                F["tb"][f] = 0.5 * (T[i, j] + gT)
                F["qn"][f] = -(gT - T[i, j]) / (pe * h)
    return out


def edge_terms(F):
    """The (8, nf) terms whose sums are the edge's record."""
    nx = np.array([float(DI[k]) for _, _, k in F["cells"]])
    ny = np.array([float(DJ[k]) for _, _, k in F["cells"]])
    ds = F["ds"]
    return np.array([ds, F["p"] * nx * ds, F["p"] * ny * ds, -(F["tx"] * ds), -(F["ty"] * ds), F["un"] * ds,
                     F["qn"] * ds, F["un"] * F["tb"] * ds]).reshape(8, len(ds))


def edge_sums(faces):
    """(n_edges, 8): the SUMS of every edge, exactly rounded."""
    return np.array([[math.fsum(row) for row in edge_terms(F)] for F in faces]).reshape(len(faces), 8)


def loads(G, dt, re, u, v, phi, scalar=None):
    """(faces, sums): face_values and their edge_sums."""
    faces = face_values(G, dt, re, u, v, phi, scalar)
    return faces, edge_sums(faces)


def sum_bounds(faces, pmax=0.0):
    """(n_edges, 8): what any summation order of an edge's nf terms may differ by from another, nf 2^-52 sum |term|,
    plus 1e-12 pmax len on fpx / fpy (the pressure column's own bar)."""
    out = np.zeros((len(faces), 8))
    for e, F in enumerate(faces):
        t = edge_terms(F)
        out[e] = len(F["ds"]) * 2.0 ** -52 * np.array([math.fsum(np.abs(row)) for row in t])
        out[e, 1:3] += 1e-12 * pmax * math.fsum(F["ds"])
    return out
