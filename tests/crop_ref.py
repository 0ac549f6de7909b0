"""NumPy / pure-Python restatement of the square-crop contract of include/sr355.h (csrc/crop.hip), and of the thing the contract replaces: a
Suzuki-Abe outer-border follower with the shoelace area, i.e. what findContours(RETR_EXTERNAL) + contourArea + boundingRect compute.
tests/test_crop_cpu.py checks that the two agree; tests/test_crop_gpu.py checks the device against this file.  Needs neither scipy nor cv2."""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)


def gray(bgr):
    """COLOR_BGR2GRAY, 8-bit: (1868 B + 9617 G + 4899 R + 8192) >> 14."""
    a = np.asarray(bgr).astype(np.int64)
    return ((1868 * a[..., 0] + 9617 * a[..., 1] + 4899 * a[..., 2] + 8192) >> 14).astype(np.uint8)


def otsu_from_hist(h):
    """OpenCV 4's getThreshVal_Otsu_8u on 256 counts, in float64, one rounding per operation."""
    h = [int(v) for v in h]
    scale = 1.0 / float(sum(h))
    mu = 0.0
    for i in range(256):
        mu += float(i) * float(h[i])
    mu *= scale
    mu1 = q1 = 0.0
    max_sigma, max_val = 0.0, 0
    for i in range(256):
        p = float(h[i]) * scale
        mu1 *= q1
        q1 += p
        q2 = 1.0 - q1
        if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1.0 - FLT_EPSILON:
            continue
        mu1 = (mu1 + float(i) * p) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma, max_val = sigma, i
    return max_val


def otsu(gray_u8):
    return otsu_from_hist(np.bincount(np.asarray(gray_u8).ravel(), minlength=256))


_N4 = ((0, 1), (1, 0), (0, -1), (-1, 0))
_N8 = _N4 + ((1, 1), (1, -1), (-1, -1), (-1, 1))


def label(mask, connectivity):
    """Flood fill: int32 [H, W], every True pixel labelled with the smallest raster index y W + x of its component, -1 elsewhere."""
    m = np.asarray(mask, bool)
    H, W = m.shape
    nb = _N4 if connectivity == 4 else _N8
    out = np.full((H, W), -1, np.int32)
    todo = m.copy()
    for y0, x0 in zip(*np.nonzero(m)):                   # raster order: a component is first met at its smallest index
        if not todo[y0, x0]:
            continue
        seed = int(y0) * W + int(x0)
        todo[y0, x0] = False
        stack = [(int(y0), int(x0))]
        while stack:
            y, x = stack.pop()
            out[y, x] = seed
            for dy, dx in nb:
                v, u = y + dy, x + dx
                if 0 <= v < H and 0 <= u < W and todo[v, u]:
                    todo[v, u] = False
                    stack.append((v, u))
    return out


def fill_holes(mask):
    """F = not outside, outside the 4-connected background component of the one-pixel ring of background around the frame."""
    m = np.asarray(mask, bool)
    pad = np.zeros((m.shape[0] + 2, m.shape[1] + 2), bool)
    pad[1:-1, 1:-1] = m
    bg = label(~pad, 4)
    return ~(bg == bg[0, 0])[1:-1, 1:-1]


def cell_area2(comp):
    """Twice the contour area of one component (bool [H, W]): 2 per 2 x 2 cell with four of its pixels, 1 per cell with three."""
    c = np.asarray(comp).astype(np.int64)
    n = c[:-1, :-1] + c[:-1, 1:] + c[1:, :-1] + c[1:, 1:]
    return int(2 * (n == 4).sum() + (n == 3).sum())


def pixel_bbox(comp):
    ys, xs = np.nonzero(comp)
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


# the 8 neighbours counter-clockwise as seen on the screen (y down), starting east
_CCW = ((0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))


def trace_outer_border(comp):
    """Suzuki-Abe border following of the outer border of one 8-connected component (bool [H, W]), started where the raster scan meets it.
    -> list of (x, y) border points in the order followed (no approximation: CHAIN_APPROX_SIMPLE drops collinear points only, which changes
    neither the area nor the bounding rectangle)."""
    c = np.pad(np.asarray(comp, bool), 1)
    ys, xs = np.nonzero(c)
    i, j = int(ys[0]), int(xs[0])                        # first pixel in raster order: its west neighbour is background
    start = _CCW.index((0, -1))
    first = None
    for k in range(1, 9):                                # clockwise from west
        d = _CCW[(start - k) % 8]
        if c[i + d[0], j + d[1]]:
            first = (i + d[0], j + d[1])
            break
    if first is None:
        return [(j - 1, i - 1)]
    pts = []
    i2, j2 = first
    i3, j3 = i, j
    while True:
        s = _CCW.index((i2 - i3, j2 - j3))
        for k in range(1, 9):                            # counter-clockwise from the element after (i2, j2)
            d = _CCW[(s + k) % 8]
            if c[i3 + d[0], j3 + d[1]]:
                i4, j4 = i3 + d[0], j3 + d[1]
                break
        pts.append((j3 - 1, i3 - 1))
        if (i4, j4) == (i, j) and (i3, j3) == first:
            return pts
        i2, j2 = i3, j3
        i3, j3 = i4, j4


def shoelace_area2(pts):
    """Twice contourArea of a closed polygon of integer points."""
    a = 0
    for k in range(len(pts)):
        x0, y0 = pts[k - 1]
        x1, y1 = pts[k]
        a += x0 * y1 - x1 * y0
    return abs(a)


def points_bbox(pts):
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    return min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1


def crop_origin(W, H, rect):
    """(left, top) of the S x S square, S = min(W, H): centred on rect = (x, y, ww, hh) and pulled back into the frame; rect None: centred."""
    S = min(W, H)
    if rect is None:
        return (W - S) // 2, (H - S) // 2
    x, y, ww, hh = rect
    cx, cy = x + ww // 2, y + hh // 2
    left, top = max(0, cx - S // 2), max(0, cy - S // 2)
    if left + S > W:
        left = W - S
    if top + S > H:
        top = H - S
    return max(0, left), max(0, top)


def winner(labels):
    """Root of the component with the largest area; among equal areas the largest root.  None without a component.  -> (root, rect)"""
    best = None
    for r in np.unique(labels[labels >= 0]):
        key = (cell_area2(labels == r), int(r))
        if best is None or key > best:
            best = key
    if best is None:
        return None, None
    return best[1], pixel_bbox(labels == best[1])


def boxes_from_mask(mask):
    """mask bool [H, W] -> (row [found, x, y, ww, hh, left, top] as a list, labels of F)."""
    H, W = mask.shape
    labels = label(fill_holes(mask), 8)
    root, rect = winner(labels)
    left, top = crop_origin(W, H, rect)
    return [int(rect is not None)] + list(rect or (0, 0, 0, 0)) + [left, top], labels


def object_boxes(frames):
    """uint8 BGR [B, H, W, 3] -> dict: 'boxes' int32 [B, 8] {found, x, y, ww, hh, left, top, otsu_t}, 'gray' uint8, 'mask' uint8 (0 / 255),
    'labels' int32 [B, H, W]."""
    frames = np.asarray(frames)
    g = gray(frames)
    boxes, masks, labels = [], [], []
    for b in range(frames.shape[0]):
        t = otsu(g[b])
        m = g[b] > t
        row, lab = boxes_from_mask(m)
        boxes.append(row + [t])
        masks.append(np.where(m, 255, 0).astype(np.uint8))
        labels.append(lab)
    return {"boxes": np.asarray(boxes, np.int32), "gray": g, "mask": np.stack(masks), "labels": np.stack(labels)}


def square_crop(frames, boxes):
    frames = np.asarray(frames)
    S = min(frames.shape[1], frames.shape[2])
    return np.stack([f[int(r[6]):int(r[6]) + S, int(r[5]):int(r[5]) + S] for f, r in zip(frames, boxes)])


# ---------------------------------------------------------------------------------------------- named shapes (bool masks)
def frames_from_mask(mask):
    """A BGR frame whose gray is 255 on the mask and 0 off it: Otsu's threshold is then 0 (or the frame constant) and the mask is the design."""
    m = np.asarray(mask, bool)
    return np.repeat(np.where(m, 255, 0).astype(np.uint8)[..., None], 3, axis=-1)


def checkerboard(H, W):
    yy, xx = np.mgrid[:H, :W]
    return (yy + xx) % 2 == 0


def spiral(H, W, gap=2):
    """A one-pixel rectangular spiral wound inward with `gap` background pixels between its turns: one long 4-connected line through every tile."""
    m = np.zeros((H, W), bool)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    step = gap + 1
    first = True
    while top <= bottom and left <= right:
        m[top, (left if first else max(left - step, 0)):right + 1] = True
        m[top:bottom + 1, right] = True
        if bottom - top < step or right - left < step:
            break
        m[bottom, left:right + 1] = True
        m[top + step:bottom + 1, left] = True
        top += step
        left += step
        bottom -= step
        right -= step
        first = False
    return m


def serpentine(H, W, pitch=3):
    """Horizontal one-pixel lines every `pitch` rows joined alternately at the right and the left end: one component snaking over every seam."""
    m = np.zeros((H, W), bool)
    rows = list(range(0, H, pitch))
    for k, y in enumerate(rows):
        m[y, :] = True
        if k + 1 < len(rows):
            m[y:rows[k + 1] + 1, W - 1 if k % 2 == 0 else 0] = True
    return m


def nested_rings(H, W, n=4, width=2, gap=3):
    m = np.zeros((H, W), bool)
    for k in range(n):
        o = 1 + k * (width + gap)
        if H - 2 * o < 2 * width + 1 or W - 2 * o < 2 * width + 1:
            break
        m[o:H - o, o:W - o] = True
        m[o + width:H - o - width, o + width:W - o - width] = False
    return m
