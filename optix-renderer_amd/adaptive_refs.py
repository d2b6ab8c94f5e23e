"""fp32 numpy restatement of the reference's adaptive sampler and of the render loop it drives.

Written from src/samplers/adaptive.cpp, the adaptive branch of renderThreadMain and renderBlock
(src/utils/render.cpp:266, :323-336, :421-459), computeVarianceFromImage (src/utils/common.cpp:339-398),
DiscretePDF (include/nori/dpdf.h), ImageBlock::put and BlockGenerator (src/utils/block.cpp), in the reference's
single-thread serial order: outer sample, then block in spiral order, then pass. It is the comparison the GPU tests
make bit for bit (tests/test_gpu_adaptive.py); DESIGN.md section 7c lists the quirks it keeps.

What cannot be replayed follows DESIGN.md section 3: a path takes the per-path stream of pixel index y W + x and sample
index (s 1002 + k) 16 + i (outer sample s, pass k, path i) -- `path_fn(x, y, sample)` returns its radiance and pixel
jitter, OracleScene.path with the seed bound -- and only the index draws use the block's own pcg32 stream. Eigen's
sum() / squaredNorm() are restated as the linear vectorised redux of Eigen 3.3.8 with SSE2 packets (eigen_redux_sum),
pinned to a recording (tests/golden/adaptive_eigen_redux.json).
"""
from __future__ import annotations

import base64
import bisect
import gzip
import json
import os

import numpy as np

f32 = np.float32
BLOCK = 4                  # NORI_BLOCK_SIZE_ADAPTIVE (block.h:31)
PASS_STRIDE = 1002         # sample indices per outer sample: a block runs at most 1001 passes
PATHS_PER_PASS = 16
MAX_ROUND = 1000           # adaptive.cpp:78
EPS = f32(1e-4)
_M64 = (1 << 64) - 1
_PCG_MULT = 0x5851F42D4C957F2D


_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES_FIXTURE = os.path.join(_REPO, "tests", "golden", "adaptive_scenes.json.gz")
DISNEY_SPHERE_XML = "scenes/project/disney/disney_sphere.xml"
DISNEY_TEST_XML = "scenes/project/disney/disney-test.xml"


def materialize(out_dir: str) -> str:
    """Write the reference's two adaptive-sampler scenes (tests/golden/adaptive_scenes.json.gz: the XML files as they
    are, their mesh and images as small stand-ins, tests/golden/make_adaptive_fixture.py) under out_dir."""
    with gzip.open(SCENES_FIXTURE, "rt") as f:
        files = json.load(f)
    for rel, text in files.items():
        p = os.path.join(out_dir, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as g:
            g.write(base64.b64decode(text["base64"]) if isinstance(text, dict) else text.encode())
    return out_dir


def max_sample_count() -> int:
    """The largest outer sample count whose path sample indices stay inside int32."""
    return ((1 << 31) // PATHS_PER_PASS - (PASS_STRIDE - 1)) // PASS_STRIDE


def clamp_initial_uniform(initial_uniform: int, sample_count: int) -> int:
    """clamp(initialUniform, 1, sampleCount) (adaptive.cpp:21; Nori's clamp: lower bound first)."""
    return 1 if initial_uniform < 1 else (sample_count if initial_uniform > sample_count else initial_uniform)


class Pcg32:
    """pcg32 (ext/pcg32/pcg32.h): seed(initstate, initseq), nextUInt, nextFloat."""

    def __init__(self, initstate: int, initseq: int):
        self.state = 0
        self.inc = ((initseq << 1) | 1) & _M64
        self.next_uint()
        self.state = (self.state + initstate) & _M64
        self.next_uint()

    def next_uint(self) -> int:
        old = self.state
        self.state = (old * _PCG_MULT + self.inc) & _M64
        xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        return ((xs >> rot) | (xs << ((-rot) & 31))) & 0xFFFFFFFF

    def next_float(self) -> np.float32:
        u = np.array([(self.next_uint() >> 9) | 0x3F800000], np.uint32)
        return f32(u.view(np.float32)[0] - f32(1.0))


def spiral_blocks(width: int, height: int, bs: int = BLOCK):
    """BlockGenerator (block.cpp:151-199): [(offset x, offset y, size x, size y)] in the order next() hands out."""
    nbx = int(np.ceil(f32(width) / f32(bs)))
    nby = int(np.ceil(f32(height) / f32(bs)))
    left = nbx * nby
    bx, by = nbx // 2, nby // 2
    direction, steps_left, num_steps = 0, 1, 1  # ERight, EDown, ELeft, EUp
    out = []
    while left > 0:
        ox, oy = bx * bs, by * bs
        out.append((ox, oy, min(bs, width - ox), min(bs, height - oy)))
        left -= 1
        if left == 0:
            break
        while True:
            if direction == 0:
                bx += 1
            elif direction == 1:
                by += 1
            elif direction == 2:
                bx -= 1
            else:
                by -= 1
            steps_left -= 1
            if steps_left == 0:
                direction = (direction + 1) % 4
                if direction in (0, 2):
                    num_steps += 1
                steps_left = num_steps
            if 0 <= bx < nbx and 0 <= by < nby:
                break
    return out


def eigen_redux_sum(v) -> np.float32:
    """Eigen 3.3.8 redux_impl<.., LinearVectorizedTraversal, NoUnrolling> (Eigen/src/Core/Redux.h) with scalar_sum_op
    over the coefficients in storage (column-major) order, Packet4f: packets of 4 from index 0 (an expression has no
    alignment offset), two accumulators over pairs of packets, accumulator 0 + accumulator 1, one more packet if an
    odd one is left, predux (a0 + a2) + (a1 + a3), then the remaining coefficients one by one. Under 4 coefficients:
    a plain left-to-right sum."""
    v = np.ascontiguousarray(v, np.float32).ravel()
    n = v.size
    aligned = n // 4 * 4
    aligned2 = n // 8 * 8
    if aligned == 0:
        res = v[0]
        for i in range(1, n):
            res = f32(res + v[i])
        return f32(res)
    p0 = v[0:4].copy()
    if aligned > 4:
        p1 = v[4:8].copy()
        for i in range(8, aligned2, 8):
            p0 = p0 + v[i:i + 4]
            p1 = p1 + v[i + 4:i + 8]
        p0 = p0 + p1
        if aligned > aligned2:
            p0 = p0 + v[aligned2:aligned2 + 4]
    res = f32(f32(p0[0] + p0[2]) + f32(p0[1] + p0[3]))
    for i in range(aligned, n):
        res = f32(res + v[i])
    return res


def eigen_squared_norm(v) -> np.float32:
    """squaredNorm() = abs2().sum(): the products, reduced like eigen_redux_sum."""
    v = np.ascontiguousarray(v, np.float32).ravel()
    return eigen_redux_sum(v * v)


def _colmajor(m: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(m.T, np.float32).ravel()


def luminance(px: np.ndarray) -> np.float32:
    """Color4f::divideByFilterWeight().getLuminance() (color.h:113-118, common.cpp:265-268)."""
    r = g = b = f32(0)
    w = px[3]
    if abs(w) > EPS:
        r, g, b = f32(px[0] / w), f32(px[1] / w), f32(px[2] / w)
    return f32(f32(f32(r * f32(0.212671)) + f32(g * f32(0.715160))) + f32(b * f32(0.072169)))


def variance_from_image(block: np.ndarray, sx: int, sy: int, border: int) -> np.ndarray:
    """computeVarianceFromImage (common.cpp:339-398) of a (sy + 2b, sx + 2b, 4) block image: (sy, sx) float32.
    std::pow(float, 2) is a double pow; 1.f / sum is a float; `col +=` rounds to float once per term."""
    lum = np.zeros((sy, sx), np.float32)
    for i in range(sy):
        for j in range(sx):
            lum[i, j] = abs(luminance(block[i + border, j + border]))
    var = np.zeros((sy, sx), np.float32)
    for i in range(sy):
        for j in range(sx):
            mean, cnt = f32(0), f32(0)
            terms = []
            for k in range(3):
                for l in range(3):
                    i_, j_ = i - 1 + k, j - 1 + l
                    if i_ < 0 or i_ > sy - 1 or j_ < 0 or j_ > sx - 1:
                        continue
                    mean = f32(mean + lum[i_, j_])
                    cnt = f32(cnt + f32(1))
                    terms.append(lum[i_, j_])
            mean = f32(mean / cnt)
            inv = float(f32(f32(1) / cnt))
            col = f32(0)
            for t in terms:
                d = float(f32(t - mean))
                col = f32(float(col) + inv * (d * d))
            var[i, j] = col
    mx, mn = var.max(), var.min()
    if f32(mx - mn) < EPS:
        var[:] = 0
    else:
        for i in range(sy):
            for j in range(sx):
                var[i, j] = f32(f32(1) + f32(f32(f32(var[i, j] - mn) / f32(mx - mn)) * f32(0.254)))
    return var


class DiscretePDF:
    """include/nori/dpdf.h: append, normalize, sample."""

    def __init__(self):
        self.cdf = [f32(0)]

    def clear(self):
        self.cdf = [f32(0)]

    def size(self):
        return len(self.cdf) - 1

    def append(self, v):
        self.cdf.append(f32(self.cdf[-1] + f32(v)))

    def normalize(self):
        s = self.cdf[-1]
        if s > 0:
            norm = f32(f32(1) / s)
            for i in range(1, len(self.cdf)):
                self.cdf[i] = f32(self.cdf[i] * norm)
            self.cdf[-1] = f32(1)
        return s

    def sample(self, u) -> int:
        idx = bisect.bisect_left([float(c) for c in self.cdf], float(u))  # std::lower_bound
        return min(max(0, idx - 1), len(self.cdf) - 2)


class BlockSampler:
    """AdaptiveSampler as one block's clone (adaptive.cpp): prepare(), computeVariance(), getSampleIndices()."""

    def __init__(self, ox, oy, sx, sy, initial_uniform):
        self.sx, self.sy = sx, sy
        self.rng = Pcg32(ox, oy)  # prepare(): seeded once, never again
        self.old_var = np.zeros((sy, sx), np.float32)
        self.old_norm = f32(10000)
        self.dpdf = DiscretePDF()
        self.initial_uniform = initial_uniform
        self.round = 0
        self.stop_reason = None

    def compute_variance(self, block: np.ndarray, border: int) -> bool:
        self.stop_reason = None
        if self.round == 0:
            self.old_var[:] = 0
            self.old_norm = f32(10000)
        elif self.round == MAX_ROUND:
            self.stop_reason = "round"
            return False
        self.dpdf.clear()
        if self.round < self.initial_uniform:
            return True
        var = variance_from_image(block, self.sx, self.sy, border)
        var_diff = f32(abs(eigen_redux_sum(_colmajor(self.old_var) - _colmajor(var))))
        if abs(f32(var.max() - f32(1))) < EPS and abs(f32(var.min() - f32(1))) < EPS:  # (never true, section 7c)
            self.old_norm = var_diff
            self.old_var = var
            self.stop_reason = "ones"
            return False
        z = eigen_squared_norm(_colmajor(var))  # MatrixBase::normalize(): a zero matrix stays as it is
        if z > 0:
            var = (var / np.sqrt(z, dtype=np.float32)).astype(np.float32)
        for i in range(self.sy):
            for j in range(self.sx):
                self.dpdf.append(var[i, j])
        self.dpdf.normalize()
        if var_diff > self.old_norm:
            self.stop_reason = "norm"
            return False
        self.old_norm = var_diff
        self.old_var = var
        return True

    def sample_indices(self):
        """getSampleIndices: (first, second) pairs; renderBlock reads first as x and second as y."""
        sx, sy = self.sx, self.sy
        if self.dpdf.size() == 0:
            return [(i, j) for i in range(sy) for j in range(sx)], False
        out = []
        for _ in range(sx * sy):
            elem = self.dpdf.sample(self.rng.next_float())
            out.append((elem // sx, elem % sx))
        return out, True


def block_put(block: np.ndarray, flt, ox, oy, border, pos_x, pos_y, rgb) -> bool:
    """ImageBlock::put(pos, value) (block.cpp:93-123) into a block at offset (ox, oy)."""
    rgb = np.asarray(rgb, np.float32)
    if not (np.all(np.isfinite(rgb)) and np.all(rgb >= 0)):
        return False
    radius, lookup, table = flt
    px = f32(f32(pos_x - f32(0.5)) - f32(ox - border))
    py = f32(f32(pos_y - f32(0.5)) - f32(oy - border))
    rows, cols = block.shape[0], block.shape[1]
    x0, y0 = max(int(np.ceil(f32(px - radius))), 0), max(int(np.ceil(f32(py - radius))), 0)
    x1, y1 = min(int(np.floor(f32(px + radius))), cols - 1), min(int(np.floor(f32(py + radius))), rows - 1)
    if x1 < x0 or y1 < y0:
        return True
    wx = np.array([table[int(f32(abs(f32(f32(x) - px)) * lookup))] for x in range(x0, x1 + 1)], np.float32)
    wy = np.array([table[int(f32(abs(f32(f32(y) - py)) * lookup))] for y in range(y0, y1 + 1)], np.float32)
    v4 = np.array([rgb[0], rgb[1], rgb[2], 1.0], np.float32)
    block[y0:y1 + 1, x0:x1 + 1] += (v4[None, None, :] * wx[None, :, None]) * wy[:, None, None]
    return True


def filter_of(desc):
    """(radius, lookup factor, table) of a scene description's reconstruction filter."""
    f = desc.filter
    return f32(f.radius), f32(f.lookup_factor), np.array(f.table[:], np.float32)


class AdaptiveRender:
    """The adaptive branch of renderThreadMain over outer samples, one thread. render() may be called for
    consecutive ranges; samplers and their streams live across calls, as the reference's samplers vector does."""

    def __init__(self, width, height, flt, border, initial_uniform, path_fn):
        self.W, self.H, self.flt, self.border = width, height, flt, border
        self.path_fn = path_fn
        self.blocks = spiral_blocks(width, height)
        self.samplers = [BlockSampler(ox, oy, sx, sy, initial_uniform) for ox, oy, sx, sy in self.blocks]
        self.master = np.zeros((height + 2 * border, width + 2 * border, 4), np.float32)
        self.total_samples = 0
        self.passes = 0
        self.max_passes = 0
        self.invalid = 0
        self.log = []  # (outer sample, block, passes, stop reason, adaptive passes, elements of each adaptive pass)

    def render(self, s0: int, s1: int):
        b = self.border
        for s in range(s0, s1):
            for bi, (ox, oy, sx, sy) in enumerate(self.blocks):
                smp = self.samplers[bi]
                block = np.zeros((sy + 2 * b, sx + 2 * b, 4), np.float32)
                count = 0
                smp.round = 0
                k = 0
                picks = []
                while smp.compute_variance(block, b):
                    pairs, adaptive = smp.sample_indices()
                    self.total_samples += sx * sy
                    if adaptive:
                        picks.append([p * sx + q for p, q in pairs])
                    block[:] = 0
                    for i, (first, second) in enumerate(pairs):
                        x, y = first + ox, second + oy
                        rgb, jit = self.path_fn(x, y, (s * PASS_STRIDE + k) * PATHS_PER_PASS + i)
                        if not block_put(block, self.flt, ox, oy, b, f32(f32(x) + f32(jit[0])),
                                         f32(f32(y) + f32(jit[1])), rgb):
                            self.invalid += 1
                    self.master[oy:oy + sy + 2 * b, ox:ox + sx + 2 * b] += block
                    smp.round = count
                    count += 1
                    k += 1
                self.passes += k
                self.max_passes = max(self.max_passes, k)
                self.log.append((s, bi, k, smp.stop_reason, len(picks), picks))
        return self.master

    def stats(self) -> dict:
        return {"total_samples": self.total_samples, "passes": self.passes, "max_passes": self.max_passes,
                "n_blocks": len(self.blocks)}

    def variance(self) -> np.ndarray:
        """m_oldVariance of every block at its place in the image (writeVarianceMatrix): (H, W) float32."""
        out = np.zeros((self.H, self.W), np.float32)
        for (ox, oy, sx, sy), smp in zip(self.blocks, self.samplers):
            out[oy:oy + sy, ox:ox + sx] = smp.old_var
        return out


def for_scene(scene, oracle_scene, seed: int) -> AdaptiveRender:
    """The restatement of a loaded adaptive-sampler scene, paths from the CPU oracle at `seed`."""
    d = scene.desc
    return AdaptiveRender(d.camera.width, d.camera.height, filter_of(d), d.filter.border, d.adaptive_initial_uniform,
                          lambda x, y, smp: oracle_scene.path(seed, x, y, smp))
