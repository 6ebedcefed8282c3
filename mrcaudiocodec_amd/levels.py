"""
LevelMap: how loud every stretch of a set of `.pac` files is, from one number per block and channel -- the block energies of
mrc_pac_store_block_energy (PacStore.levels) -- and what a crop loader asks of it: the energy and RMS level of any window,
the starts whose window is loud enough, a reproducible draw among them, the gain that brings a crop to a target level, the
gain that puts one crop at a given SNR under another.
Pure NumPy: no GPU, no library call.

The windowed MDCT of the codec is an orthogonal lapped transform, so block i of shape (a_i, b_i) at position p_i of the padded
plane holds e_i = ((a_i + b_i) / D) * sum of its first (a_i + b_i) / (2 D) decoded lines squared of the decoded signal's
energy at 1 / D of the sample rate, and the e_i of a channel add up to the sum of squares of its whole overlap-added plane.
WHERE in time a block's energy lies the lines do not say; the map spreads it evenly over the block's tile

    tile_i = [(p_i + a_i / 2 - L) / D, (p_i + a_i + b_i / 2 - L) / D)

in the coordinates of PacStore.decode_window at that divisor (output samples, the MDCT's delay of L = n_mdct_lines removed):
from the middle of the block's first overlap half to the middle of its second.  Tiles abut and partition time, because
p_{i+1} = p_i + a_i and a_{i+1} = b_i; their edges are exact halves and are kept as float64.  F(t), the cumulative energy, is
piecewise linear over the tile edges, and a window's energy is F(start + window) - F(start): exact in total, local to within
the blocks it cuts.  (A window of a second is good to a few hundredths of a dB, one of 16 384 samples to a few tenths; a
window as short as a few blocks can be tens of dB off beside a much louder block: DESIGN.md, "Block energies".)

Levels are dB re a full-scale signed fraction of 1.0: 10 log10(energy / window), -inf for digital silence.
"""
import numpy as np


def _db(power):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(power)


class LevelMap:
    """files: per file a dict(blocks=[n_blocks][3] (block_start, a, b: full rate, padded plane, as pacfile.index gives them),
    energy=[n_blocks][channels] (PacStore.levels: at rate 1 / D), n_samples=the file's samples per channel at rate 1 / D).
    L = n_mdct_lines, D the rate divisor the energies were taken at, n_short the short block length (the default grid of
    starts is n_short / D).  A file's blocks must follow one another (ValueError otherwise).
    .channels: the largest channel count among the files; a file of fewer channels repeats its channel in every result."""

    def __init__(self, files, L, D=1, n_short=None):
        self.L, self.D = int(L), int(D)
        self.n_short = int(n_short) if n_short is not None else None
        if self.D < 1 or self.L % self.D or (self.n_short is not None and (self.n_short < self.D or self.n_short % self.D)):
            raise ValueError("LevelMap: D = %d must divide n_mdct_lines = %d and n_short = %r" % (self.D, self.L, n_short))
        self.n_samples, self.edges, self.cum, self.energy = [], [], [], []
        for f, item in enumerate(files):
            blocks = np.asarray(item["blocks"], dtype=np.int64).reshape(-1, 3)
            energy = np.asarray(item["energy"], dtype=np.float64)
            if energy.ndim != 2:
                energy = energy.reshape(len(blocks), -1) if len(blocks) else np.zeros((0, 1))
            if energy.shape[0] != len(blocks) or energy.shape[1] < 1 or not np.all(energy >= 0.0):
                raise ValueError("LevelMap: file %d: energies must be [n_blocks][channels >= 1] and >= 0" % f)
            p, a, b = blocks[:, 0], blocks[:, 1], blocks[:, 2]
            if len(blocks) > 1 and not (np.array_equal(p[1:], p[:-1] + a[:-1]) and np.array_equal(a[1:], b[:-1])):
                raise ValueError("LevelMap: file %d: blocks do not follow one another (p' = p + a, a' = b)" % f)
            edges = np.zeros(len(blocks) + 1) if len(blocks) else np.zeros(1)
            if len(blocks):
                edges[:-1] = (p + a / 2.0 - self.L) / self.D                  # exact: halves of integers over 1, 2 or 4
                edges[-1] = (p[-1] + a[-1] + b[-1] / 2.0 - self.L) / self.D
                assert np.all(np.diff(edges) > 0) and np.array_equal(edges[1:-1], ((p + a + b / 2.0 - self.L) / self.D)[:-1])
            cum = np.zeros((energy.shape[1], len(edges)))
            np.cumsum(energy.T, axis=1, out=cum[:, 1:])
            self.n_samples.append(int(item["n_samples"]))
            self.edges.append(edges)
            self.cum.append(cum)
            self.energy.append(energy)
        self.channels = max([c.shape[0] for c in self.cum], default=1)

    def __len__(self):
        return len(self.edges)

    def _file(self, f, what):
        if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or not 0 <= int(f) < len(self):
            raise ValueError("%s: file %r is not one of the map's %d files" % (what, f, len(self)))
        return int(f)

    @staticmethod
    def _window(window, what):
        if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or int(window) <= 0:
            raise ValueError("%s: window must be a positive int, got %r" % (what, window))
        return int(window)

    def _step(self, step, what):
        if step is None:
            if self.n_short is None:
                raise ValueError("%s: the map has no n_short, give step" % what)
            return self.n_short // self.D
        if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or int(step) <= 0:
            raise ValueError("%s: step must be a positive int, got %r" % (what, step))
        return int(step)

    def tiles(self, f):
        """the tile edges of file f, float64 [n_blocks + 1] (a file without blocks: one edge)"""
        return self.edges[self._file(f, "tiles")]

    def total_energy(self, f):
        """[channels of the file]: the sum of its blocks' energies"""
        return self.cum[self._file(f, "total_energy")][:, -1].copy()

    def cumulative(self, f, t):
        """F_{f,c}(t) -> [len(t)][channels]: 0 before the first tile, the file's total behind the last"""
        f = self._file(f, "cumulative")
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        cum = self.cum[f]
        out = np.empty((t.size, self.channels))
        for c in range(self.channels):
            out[:, c] = np.interp(t, self.edges[f], cum[min(c, cum.shape[0] - 1)])
        return out

    def _energy(self, f, starts, window):
        starts = np.asarray(starts, dtype=np.float64).reshape(-1)
        return self.cumulative(f, starts + window) - self.cumulative(f, starts)

    def window_energy(self, files, starts, window):
        """-> [n][channels]: F(start + window) - F(start) of each (file, start); zero outside the tiles"""
        window = self._window(window, "window_energy")
        files = np.asarray(files, dtype=np.int64).reshape(-1)
        starts = np.asarray(starts, dtype=np.int64).reshape(-1)
        if files.shape != starts.shape:
            raise ValueError("window_energy: one start per file index (%d files, %d starts)" % (files.size, starts.size))
        out = np.zeros((files.size, self.channels))
        for f in np.unique(files):
            sel = files == f
            out[sel] = self._energy(self._file(int(f), "window_energy"), starts[sel], window)
        return out

    def window_rms_db(self, files, starts, window):
        """-> [n][channels]: 10 log10(window_energy / window), dB re full scale, -inf where the window is silent"""
        return _db(self.window_energy(files, starts, window) / self._window(window, "window_rms_db"))

    def grid(self, f, window, step=None):
        """the starts 0, step, 2 step, ... <= n_samples - window of file f (none if the file is shorter than the window)"""
        f, window, step = self._file(f, "grid"), self._window(window, "grid"), self._step(step, "grid")
        return np.arange(0, self.n_samples[f] - window + 1, step, dtype=np.int64)

    def grid_levels(self, f, window, step=None):
        """-> (starts, dB [len(starts)]): the loudest channel's window level at every start of the grid"""
        starts = self.grid(f, window, step)
        return starts, _db(self._energy(f, starts, window).max(axis=1) / window) if starts.size else np.zeros(0)

    def admissible_starts(self, f, window, min_rms_db, step=None):
        """the starts of the grid whose loudest channel's window level is at least min_rms_db"""
        starts, db = self.grid_levels(f, window, step)
        return starts[db >= float(min_rms_db)]

    def sample_starts(self, files, window, min_rms_db, rng, step=None, fallback=None):
        """one start per item, drawn uniformly from that file's admissible starts with the numpy.random.Generator rng (one
        call of rng.integers for all items: the same generator state gives the same starts).  A file without an admissible
        start is a ValueError naming it; with fallback="loudest" it gives the start of its loudest window instead (the first
        on ties; 0 for a file shorter than the window)."""
        if fallback not in (None, "loudest"):
            raise ValueError('sample_starts: fallback must be None or "loudest", got %r' % (fallback,))
        if not isinstance(rng, np.random.Generator):
            raise ValueError("sample_starts: rng must be a numpy.random.Generator")
        files = np.asarray(files, dtype=np.int64).reshape(-1)
        choices = {}
        for f in np.unique(files):
            f = self._file(int(f), "sample_starts")
            starts, db = self.grid_levels(f, window, step)
            ok = starts[db >= float(min_rms_db)]
            if not ok.size:
                if fallback is None:
                    raise ValueError("sample_starts: file %d has no window of %d samples at or above %g dB" % (f, window, min_rms_db))
                ok = starts[np.argmax(db):][:1] if starts.size else np.zeros(1, np.int64)
            choices[f] = ok
        counts = np.array([choices[int(f)].size for f in files], dtype=np.int64)
        draw = rng.integers(0, counts) if files.size else np.zeros(0, np.int64)
        return np.array([choices[int(f)][k] for f, k in zip(files, draw)], dtype=np.int64)

    def gains_to(self, target_rms_db, files, starts, window):
        """-> [n] linear factors that bring each window's loudest channel to target_rms_db; 1.0 where the window is silent"""
        energy = self.window_energy(files, starts, window).max(axis=1)
        gain = np.ones(energy.size)
        loud = energy > 0.0
        gain[loud] = 10.0 ** ((float(target_rms_db) - _db(energy[loud] / window)) / 20.0)
        return gain

    def gains_for_snr(self, snr_db, files_a, starts_a, files_b, starts_b, window):
        """-> [n] linear factors g for the b windows such that a + g * b has the a window snr_db above the b window: with E the
        window energy summed over the channels, g = sqrt(E_a / (E_b * 10 ** (snr_db / 10))).  1.0 where either window is
        silent: no SNR is defined there.  The factors PacStore.decode_window_sum takes for the b terms, the a terms at 1.0."""
        e_a = self.window_energy(files_a, starts_a, window).sum(axis=1)
        e_b = self.window_energy(files_b, starts_b, window).sum(axis=1)
        if e_a.shape != e_b.shape:
            raise ValueError("gains_for_snr: one b window per a window (%d and %d)" % (e_a.size, e_b.size))
        gain = np.ones(e_a.size)
        both = (e_a > 0.0) & (e_b > 0.0)
        gain[both] = np.sqrt(e_a[both] / (e_b[both] * 10.0 ** (float(snr_db) / 10.0)))
        return gain
