"""Host restatement of the SEATED mix-matrix bank (include/dspfx.h, dspfx_mixmatrix_create_seats / _assign), for the seat tests.
Written from the rule in the header, not from the product code.

A room owns S_r seats (a multiple of 32) and an S_r x S_r matrix M[l][s] indexed by seat; a channel holds one seat of one room or
none (NONE).  At first channel c0 + i of room r sits in seat i, and the matrix holds mix-minus among the taken seats; every entry
in the row or the column of an empty seat is +0.0, always.

THE SEATING RULE of one assign(ids, first_channel): the range, every id and every room's capacity are checked first (Refused, and
nothing changes).  A channel whose id is its current room is untouched.  All other named channels first leave: their seat is
free, its row and column become +0.0.  Then the channels that enter a room do so in ascending channel order, each into the lowest
free seat.  A newcomer's row and column, by the seating after the whole call: MIX_MINUS: 1.0 at every other taken seat, +0.0 on
the diagonal and at empty seats; ZERO: +0.0.  Entries between two channels that both stayed are not touched.

gathered() turns a seated problem into the contiguous one an unseated bank (and mixmatrix_ref) can be applied to as they are: a
block of sum S_r channels in seat order with +0.0 columns at the empty seats, and the table [0, S_0, S_0 + S_1, ..]."""
import numpy as np

NONE = 0xFFFFFFFF
MIX_MINUS, ZERO = 0, 1


class Refused(Exception):
    """what: "range", "id" or "capacity" """

    def __init__(self, what, detail=""):
        super().__init__(f"{what}: {detail}")
        self.what = what


def round32(v):
    return (np.asarray(v, np.int64) + 31) // 32 * 32


def initial(table, seats):
    """-> (room_of, seat_of) int64[N] of a fresh bank; seats are checked against the members"""
    gs = [int(v) for v in table]
    S = round32(seats)
    room_of, seat_of = np.zeros(gs[-1], np.int64), np.zeros(gs[-1], np.int64)
    for g, (a, b) in enumerate(zip(gs[:-1], gs[1:])):
        assert b - a <= S[g]
        room_of[a:b] = g
        seat_of[a:b] = np.arange(b - a)
    return room_of, seat_of


def reseat(room_of, seat_of, seats, ids, first=0):
    """The rule on arrays -> (room_of, seat_of, moves) as new arrays; moves = [(channel, old room, old seat, new room, new seat)]
    in ascending channel order.  Refused when the call is bad; the inputs are never changed."""
    room_of, seat_of = np.array(room_of, np.int64), np.array(seat_of, np.int64)
    S = round32(seats)
    N, G = len(room_of), len(S)
    ids = [int(v) for v in np.atleast_1d(ids)]
    if len(ids) == 0 or first < 0 or first >= N or first + len(ids) > N:
        raise Refused("range", f"[{first}, {first} + {len(ids)}) of {N}")
    for i, g in enumerate(ids):
        if g != NONE and not 0 <= g < G:
            raise Refused("id", f"channel {first + i} -> {g}")
    movers = [(first + i, g) for i, g in enumerate(ids) if g != room_of[first + i]]
    occ = np.bincount(room_of[room_of != NONE], minlength=G)
    for c, g in movers:
        if room_of[c] != NONE:
            occ[room_of[c]] -= 1
        if g != NONE:
            occ[g] += 1
    if (occ > S).any():
        raise Refused("capacity", f"room {int(np.argmax(occ > S))}")
    taken = [set(seat_of[room_of == g].tolist()) for g in range(G)]
    assert sum(len(t) for t in taken) == (room_of != NONE).sum()          # no seat is held twice
    moves = []
    for c, g in movers:                                   # the leaves
        moves.append([c, int(room_of[c]), int(seat_of[c]), g, NONE])
        if room_of[c] != NONE:
            taken[room_of[c]].remove(int(seat_of[c]))
        room_of[c], seat_of[c] = NONE, NONE
    for m in moves:                                       # the enters: ascending channel, the lowest free seat
        c, g = m[0], m[3]
        if g == NONE:
            continue
        q = next(s for s in range(int(S[g])) if s not in taken[g])
        taken[g].add(q)
        room_of[c], seat_of[c] = g, q
        m[4] = q
    return room_of, seat_of, [tuple(m) for m in moves]


class Bank:
    """The host model of a seated bank: the seating and the matrices mats[r][l][s] (float32, by seat)."""

    def __init__(self, table, seats):
        self.table = [int(v) for v in table]
        self.S = round32(seats)
        self.N, self.G = self.table[-1], len(self.S)
        self.room_of, self.seat_of = initial(table, seats)
        self.mats = [np.zeros((int(s), int(s)), np.float32) for s in self.S]
        for g in range(self.G):
            self.fill(g, MIX_MINUS)

    def chan(self, g):
        """int64[S_g]: the channel in every seat of room g (NONE: empty)"""
        out = np.full(int(self.S[g]), NONE, np.int64)
        for c in np.nonzero(self.room_of == g)[0]:
            out[self.seat_of[c]] = c
        return out

    def occupancy(self):
        return np.bincount(self.room_of[self.room_of != NONE], minlength=self.G)

    def fill(self, g, preset):
        t = self.chan(g) != NONE
        self.mats[g][:] = 0.0
        if preset == MIX_MINUS:
            self.mats[g][np.ix_(t, t)] = 1.0
            np.fill_diagonal(self.mats[g], 0.0)

    def assign(self, ids, first=0, preset=MIX_MINUS):
        room_of, seat_of, moves = reseat(self.room_of, self.seat_of, self.S, ids, first)
        self.room_of, self.seat_of = room_of, seat_of
        for _, r0, q0, _, _ in moves:
            if r0 != NONE:
                self.mats[r0][q0, :] = 0.0
                self.mats[r0][:, q0] = 0.0
        for _, _, _, r1, q1 in moves:                     # by the seating after the whole call
            if r1 == NONE:
                continue
            line = ((self.chan(r1) != NONE) & (np.arange(int(self.S[r1])) != q1)).astype(np.float32)
            self.mats[r1][q1, :] = line if preset == MIX_MINUS else 0.0
            self.mats[r1][:, q1] = line if preset == MIX_MINUS else 0.0
        return moves

    def set_lines(self, values, first, cols=False):
        """set_rows / set_cols: values[count][S_r] by seat for channels first .., which share a room; empty seats take +0.0"""
        values = np.asarray(values, np.float32)
        g = int(self.room_of[first])
        assert g != NONE and (self.room_of[first:first + len(values)] == g).all() and values.shape[1] == self.S[g]
        t = self.chan(g) != NONE
        for i, v in enumerate(values):
            q = int(self.seat_of[first + i])
            if cols:
                self.mats[g][:, q] = np.where(t, v, np.float32(0.0))
            else:
                self.mats[g][q, :] = np.where(t, v, np.float32(0.0))

    def set_pairs(self, listeners, sources, gains):
        for l, s, v in zip(listeners, sources, gains):
            g = int(self.room_of[l])
            assert g != NONE and g == self.room_of[s]
            self.mats[g][self.seat_of[l], self.seat_of[s]] = np.float32(v)

    def gtable(self):
        return [0] + [int(v) for v in np.cumsum(self.S)]

    def gathered(self, x):
        return gathered(x, self.room_of, self.seat_of, self.S)

    def scatter(self, yg):
        """the gathered problem's output [F][sum S] -> [F][N] by channel; +0.0 for a channel in no room"""
        yg = np.asarray(yg)
        off = self.gtable()
        out = np.zeros((yg.shape[0], self.N), yg.dtype)
        for c in range(self.N):
            if self.room_of[c] != NONE:
                out[:, c] = yg[:, off[self.room_of[c]] + self.seat_of[c]]
        return out

    def occupied_of(self):
        """float64[sum S]: per gathered channel the taken seats of its room (the n of the error bound)"""
        return np.repeat(self.occupancy().astype(np.float64), self.S)


def gathered(x, room_of, seat_of, seats):
    """x [F][N] -> (xg [F][sum S] f32: the sample of the channel in every seat, +0.0 at empty seats; table [0, S_0, S_0 + S_1, ..])"""
    x = np.asarray(x, np.float32)
    S = round32(seats)
    off = [0] + [int(v) for v in np.cumsum(S)]
    xg = np.zeros((x.shape[0], off[-1]), np.float32)
    for c in range(x.shape[1]):
        if room_of[c] != NONE:
            xg[:, off[room_of[c]] + seat_of[c]] = x[:, c]
    return xg, off
