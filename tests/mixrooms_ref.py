"""float64 restatement of the mix-group bank in mapped mode (include/dspfx.h, dspfx_mixgroups_assign), for the seating tests.
Written from the contract in the header, not from the product code: "group g" is {c : room_of[c] == g}, an unseated channel
(NO_ROOM) is in no sum and its return is +0.0, a room of one gets +0.0, an empty room's bus is +0.0.  The terms are formed in
numpy float32 (mixgroups_ref.terms), summed in float64 and divided by the float64 value of the f32 divisor.  The bounds are
mixgroups_ref.bound with the depth D that dspfx_mixgroups_room_plan reports: D for a bus, D + 1 for a return (the
subtraction); they hold no measured constant."""
import numpy as np

from mixgroups_ref import bound, cap, link_divisor, terms  # noqa: F401  (re-exported for the tests)

NO_ROOM = 0xFFFFFFFF


def members(room_of, groups):
    """-> list of int64 arrays: the channels of every room, ascending"""
    r = np.asarray(room_of, np.int64)
    return [np.flatnonzero(r == g) for g in range(groups)]


def counts(room_of, groups):
    return np.asarray([len(m) for m in members(room_of, groups)], np.int64)


def buses(x, room_of, groups, gain=None, normalise=True):
    """-> (ref [F][G] f64, sabs [F][G] f64 = sum|t| / div): an empty room gives 0 in both.  Only finite members are summed into
    sabs and ref when the caller masks them; a NaN or inf among a room's members propagates, as in the bank."""
    t = terms(x, gain).astype(np.float64)
    ref = np.zeros((t.shape[0], groups))
    sabs = np.zeros_like(ref)
    for g, m in enumerate(members(room_of, groups)):
        if len(m) == 0:
            continue
        div = float(link_divisor(len(m))) if normalise else 1.0
        with np.errstate(invalid="ignore"):
            ref[:, g] = t[:, m].sum(axis=1) / div
            sabs[:, g] = np.abs(t[:, m]).sum(axis=1) / div
    return ref, sabs


def returns_exact(x, room_of, groups, gain=None, normalise=True):
    """-> (ref [F][N] f64, sabs [F][N] f64): ref = (float64 sum of the OTHER members' f32 terms) / divisor(n_g - 1), sabs = (sum
    of |t| over the whole room) / divisor(n_g - 1); an unseated channel and a room of one give 0 in both."""
    t = terms(x, gain).astype(np.float64)
    ref = np.zeros_like(t)
    sabs = np.zeros_like(t)
    for m in members(room_of, groups):
        n = len(m)
        if n < 2:
            continue
        div = float(link_divisor(n - 1)) if normalise else 1.0
        tm = t[:, m]
        # the sum of the others, without cancellation: prefix sums from the left plus from the right
        with np.errstate(invalid="ignore"):
            left = np.concatenate([np.zeros((t.shape[0], 1)), np.cumsum(tm[:, :-1], axis=1)], axis=1)
            right = np.concatenate([np.cumsum(tm[:, :0:-1], axis=1)[:, ::-1], np.zeros((t.shape[0], 1))], axis=1)
            ref[:, m] = (left + right) / div
            sabs[:, m] = (np.abs(tm).sum(axis=1) / div)[:, None]
    return ref, sabs


def bus_bound(sabs, ref, depth):
    """depth [G] from room_plan"""
    return bound(sabs, ref, np.asarray(depth, np.float64)[None, :])


def returns_bound(sabs, ref, depth, room_of):
    """depth [G] from room_plan; a return has one rounding more than the bus, for the subtraction"""
    r = np.asarray(room_of, np.int64)
    d = np.zeros(len(r))
    seated = r != NO_ROOM
    d[seated] = np.asarray(depth, np.float64)[r[seated]]
    return bound(sabs, ref, d[None, :] + 1.0)
