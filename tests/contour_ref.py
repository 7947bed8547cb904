"""Restatement of the quad search of prl::documentContour (include/prl_hip.h, "document contour") for the tests: numpy and plain
Python, written from the header's text.

  find_contours     cv::findContours(RETR_CCOMP, CHAIN_APPROX_SIMPLE): [(points, is_hole)] in OpenCV's order
  approx_closed     cv::approxPolyDP(points, eps, closed=True) on integer points
  reduce_polygon    the reference's loop: eps = 1, 2, ... until at most four points remain (every step is returned)
  document_quad     findDocumentContour: four corners in the polygon's own order, or None
  quad_finish       scaleContour + cropVerticesOrdering: 8 float32
  morphology_ex     cv::morphologyEx with anchor and iterations, from nuil_ref's element, n real passes
  document_contour  the whole of prl::documentContour(page, -1, -1) from edges_ref's map: (quad or None, try)

[upstream] OpenCV 3.4 / 4.x, unpinned like the rest of the project.
"""
from __future__ import annotations

import math

import numpy as np

import edges_ref as er
import nuil_ref as nr

STEP = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))   # direction -> (dx, dy)
RIGHT_END = -126


def _trace(img, x0, y0, hole):
    """one border from the padded coordinates (x0, y0); marks img; returns the points in page coordinates"""
    def at(x, y, s):
        return img[y + STEP[s & 7][1], x + STEP[s & 7][0]]

    out = []
    first = 0 if hole else 4
    s = first
    while True:   # clockwise from `first`
        s = (s - 1) & 7
        if at(x0, y0, s) != 0 or s == first:
            break
    if s == first:
        img[y0, x0] = RIGHT_END
        return [(x0 - 1, y0 - 1)]
    x1, y1 = x0 + STEP[s][0], y0 + STEP[s][1]
    x3, y3 = x0, y0
    before = s ^ 4
    while True:
        arrival = s
        k = s
        while k < 15:
            k += 1
            if at(x3, y3, k) != 0:
                break
        s = k & 7
        if ((s - 1) & 0xFFFFFFFF) < arrival:
            img[y3, x3] = RIGHT_END
        elif img[y3, x3] == 1:
            img[y3, x3] = 2
        if s != before:
            out.append((x3 - 1, y3 - 1))
            before = s
        x4, y4 = x3 + STEP[s][0], y3 + STEP[s][1]
        if (x4, y4) == (x0, y0) and (x3, y3) == (x1, y1):
            return out
        x3, y3 = x4, y4
        s = (s + 4) & 7


def find_contours(page):
    from scipy import ndimage

    page = np.asarray(page)
    h, w = page.shape
    img = np.zeros((h + 2, w + 2), np.int8)
    img[1:-1, 1:-1] = page != 0
    component, _n = ndimage.label(img != 0, structure=np.ones((3, 3), int))
    outers, holes = [], {}   # discovery order; holes per component label
    for y in range(1, h + 1):
        prev = 0
        row = img[y]
        for x in range(1, w + 1):
            p = int(row[x])
            if p != prev:
                if prev == 0 and p == 1:
                    outers.append((int(component[y, x]), _trace(img, x, y, False)))
                    p = int(row[x])
                elif p == 0 and prev >= 1:
                    holes.setdefault(int(component[y, x - 1]), []).append(_trace(img, x - 1, y, True))
            prev = p
    out = []
    for label, pts in reversed(outers):
        out.append((pts, False))
        for pts_h in reversed(holes.get(label, [])):
            out.append((pts_h, True))
    return out


def approx_closed(points, eps):
    pts = [(int(x), int(y)) for x, y in points]
    n = len(pts)
    if n == 0:
        return []
    eps2 = float(eps) * float(eps)
    start, far, largest = 0, 0, 0.0
    for _round in range(3):
        start = (start + far) % n
        largest = 0.0
        sx, sy = pts[start]
        for j in range(1, n):
            px, py = pts[(start + j) % n]
            d = float(px - sx) * float(px - sx) + float(py - sy) * float(py - sy)
            if d > largest:
                largest, far = d, j
    written = []
    stack = []
    if largest <= eps2:
        written.append(pts[start])
    else:
        other = (start + far) % n
        stack = [(other, start), (start, other)]
    while stack:
        a, b = stack.pop()
        ax, ay = pts[a]
        dx, dy = float(pts[b][0] - ax), float(pts[b][1] - ay)
        best, split = 0.0, None
        i = (a + 1) % n
        while i != b:
            d = abs((pts[i][1] - ay) * dx - (pts[i][0] - ax) * dy)
            if d > best:
                best, split = d, i
            i = (i + 1) % n
        if (a + 1) % n == b or best * best <= eps2 * (dx * dx + dy * dy):
            written.append(pts[a])
        else:
            stack.append((split, b))
            stack.append((a, split))
    # clean-up
    m = len(written)
    dst = list(written)
    count = m
    S = dst[m - 1]
    rd = 0      # next to read
    wr = 0      # next to write

    def take():
        nonlocal rd
        v = dst[rd]
        rd = (rd + 1) % m
        return v

    P = take()
    i = 0
    while i < m and count > 2:
        E = take()
        dx, dy = float(E[0] - S[0]), float(E[1] - S[1])
        d = abs((P[0] - S[0]) * dy - (P[1] - S[1]) * dx)
        inner = (P[0] - S[0]) * (E[0] - P[0]) + (P[1] - S[1]) * (E[1] - P[1])
        if d * d <= 0.5 * eps2 * (dx * dx + dy * dy) and dx != 0 and dy != 0 and inner >= 0:
            count -= 1
            dst[wr] = S = E
            wr = (wr + 1) % m
            P = take()
            i += 2
            continue
        dst[wr] = S = P
        wr = (wr + 1) % m
        P = E
        i += 1
    return dst[:count]


def reduce_polygon(points):
    """(polygon, [every approximation in turn])"""
    cur = [(int(x), int(y)) for x, y in points]
    steps = []
    eps = 1.0
    while len(cur) > 4:
        cur = approx_closed(cur, eps)
        steps.append(list(cur))
        eps += 1.0
    return cur, steps


def contour_area(pts):
    a = 0.0
    px, py = pts[-1]
    for x, y in pts:
        a += float(px) * float(y) - float(x) * float(py)
        px, py = x, y
    return abs(a * 0.5)


def _div(a, b):
    return float(np.float64(a) / np.float64(b)) if b == 0 else a / b


def _norm(a, b):
    return math.sqrt(float(a[0] - b[0]) ** 2 + float(a[1] - b[1]) ** 2)


def _angle(a, b, c, d):
    a1 = math.atan2(float(a[1] - b[1]), float(a[0] - b[0]))
    a2 = math.atan2(float(c[1] - d[1]), float(c[0] - d[0]))
    r = (a2 - a1) * 180.0 / 3.14
    if r < 0.0:
        r += 360.0
    if r > 180.0:
        r = 360.0 - r
    return r


def _orient(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def strictly_convex(q):
    """four points in strictly convex position: no three on a line and none inside the triangle of the others"""
    q = [(int(x), int(y)) for x, y in q]
    for i in range(4):
        o = [q[j] for j in range(4) if j != i]
        t = _orient(o[0], o[1], o[2])
        if t == 0:
            return False
        signs = [_orient(o[0], o[1], q[i]), _orient(o[1], o[2], q[i]), _orient(o[2], o[0], q[i])]
        if any(s == 0 for s in signs):
            return False
        if all((s > 0) == (t > 0) for s in signs):   # inside
            return False
    return True


def document_quad(page):
    page = np.asarray(page)
    h, w = page.shape
    cols_rows = w * h
    min_area = float(cols_rows) * 0.05
    kept = None
    with np.errstate(all="ignore"):
        for pts, _hole in find_contours(page):
            poly, _ = reduce_polygon(pts)
            if len(poly) < 4:
                continue
            area = contour_area(poly)
            s1, s2, s3, s4 = _norm(poly[0], poly[1]), _norm(poly[1], poly[2]), _norm(poly[2], poly[3]), _norm(poly[3], poly[0])
            if s1 < s3:
                s1, s3 = s3, s1
            if s2 < s4:
                s2, s4 = s4, s2
            if _div(s3, s1) < 0.85 or _div(s4, s2) < 0.85:
                continue
            if _angle(poly[0], poly[1], poly[2], poly[3]) < 160.0 or _angle(poly[1], poly[2], poly[3], poly[0]) < 160.0:
                continue
            if area > cols_rows or area < min_area:
                continue
            if area > min_area:
                min_area, kept = area, poly
    if kept is None or not strictly_convex(kept):
        return None
    return kept


def quad_finish(quad, map_w, map_h, src_w, src_h):
    import itertools

    q = [(int(x), int(y)) for x, y in quad]
    if not strictly_convex(q):
        return None
    first = min(range(4), key=lambda i: q[i])   # smallest x, then smallest y
    rest = [i for i in range(4) if i != first]
    cycle = None
    for perm in itertools.permutations(rest):
        order = [first] + list(perm)
        if all(_orient(q[order[i]], q[order[(i + 1) % 4]], q[order[(i + 2) % 4]]) > 0 for i in range(4)):
            cycle = order
    assert cycle is not None
    f = np.float32
    xs, ys = f(src_w) / f(map_w), f(src_h) / f(map_h)
    px = [f(q[i][0]) * xs for i in cycle]
    py = [f(q[i][1]) * ys for i in cycle]
    best, start = None, 0
    for i in range(4):
        d = float(f(f(px[i] * px[i]) + f(py[i] * py[i])))
        if best is None or d < best:
            best, start = d, i
    out = []
    for i in range(4):
        out += [px[(start + i) % 4], py[(start + i) % 4]]
    return np.array(out, np.float32)


def _pass(a, spans, kw, kh, ax, ay, erode):
    H, W, C = a.shape
    pad = 255 if erode else 0
    p = np.full((H + kh - 1, W + kw - 1, C), pad, np.uint8)
    p[ay:ay + H, ax:ax + W] = a
    f = np.minimum if erode else np.maximum
    out = np.full_like(a, pad)
    for i, (j1, j2) in enumerate(spans):
        for j in range(j1, j2):
            f(out, p[i:i + H, j:j + W], out=out)
    return out


def morphology_ex(img, op, shape, kw, kh, ax=-1, ay=-1, iterations=1):
    """dst(y, x) = min / max of src(y + i - ay, x + j - ax) over the element; n passes per half of a composite operator"""
    a = img if img.ndim == 3 else img[:, :, None]
    ax = kw // 2 if ax < 0 else ax
    ay = kh // 2 if ay < 0 else ay
    spans = nr.element_spans(shape, kw, kh)

    def run(x, erode):
        for _ in range(iterations):
            x = _pass(x, spans, kw, kh, ax, ay, erode)
        return x

    if op == nr.ERODE:
        r = run(a, True)
    elif op == nr.DILATE:
        r = run(a, False)
    elif op == nr.OPEN:
        r = run(run(a, True), False)
    elif op == nr.CLOSE:
        r = run(run(a, False), True)
    elif op == nr.TOPHAT:
        r = nr._sat_sub(a, run(run(a, True), False))
    elif op == nr.BLACKHAT:
        r = nr._sat_sub(run(run(a, False), True), a)
    else:
        raise ValueError("unknown morphology operation")
    return r.reshape(np.shape(img))


def contour_from_map(edge_map, src_w, src_h):
    """(quad as 8 float32 or None, try) from the edge map of a src_w x src_h page"""
    levels, _w, _h = er.document_edges_geometry(src_w, src_h)
    from_w, from_h = src_w >> levels, src_h >> levels
    quad = document_quad(edge_map)
    tries = 0
    if quad is None:
        tries = 1
        quad = document_quad(morphology_ex(edge_map, nr.CLOSE, nr.RECT, 2, 2, -1, -1, 2))
    if quad is None:
        return None, tries
    return quad_finish(quad, from_w, from_h, src_w, src_h), tries


def document_contour(page):
    a = page if page.ndim == 3 else page[:, :, None]
    edge_map, _ch = er.document_edges(a)
    return contour_from_map(edge_map, a.shape[1], a.shape[0])
