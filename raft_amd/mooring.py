"""Quasi-static mooring lines for the device (include/raftx_mooring.h): the YAML ``mooring:`` section as line records,
and the affine edits of a parametric sweep's anchors and fairleads.

A record is ML_N = 16 doubles: anchor (global) 0:3, fairlead (body frame, relative to the unit's reference point) 3:6,
unstretched length 6, EA 7, submerged weight per length w 8, seabed friction CB 9 (must be 0), zeros.  Only what the
library covers is parsed -- one catenary segment per line from a ``fixed`` point (end A) to a ``vessel`` point (end B),
moorMod 0; everything else raises ``UnsupportedFOWT`` (as raft_amd.strips does for units the kernels do not cover).
"""
import numpy as np

from .strips import UnsupportedFOWT

ML_N = 16
ML_ANCHOR, ML_FAIRLEAD, ML_L, ML_EA, ML_W, ML_CB = 0, 3, 6, 7, 8, 9
ML_WJOINT, ML_CONT = 10, 15    # continuation rows of a composite line: the weight of the point at the lower end; the mark
ML_LEG = 14                    # leg rows of a bridle: the mark (field 10 of the first leg row: the junction's weight)
MAX_SEG = 4                    # rows of one composite line, or stem rows of one bridle, at most
MAX_LEG = 3                    # leg rows of one bridle, at most (and at least 2)
FLAG_BAD_LINE, FLAG_VERTICAL, FLAG_SLACK, FLAG_NO_CONVERGENCE = 1, 2, 4, 8
FLAG_GROUNDED = 64


def lines_from_design(design, rho=1025.0, g=9.81):
    """Line records [nLine,16] of ``design['mooring']`` (MoorPy's System.parseYAML for the layouts the library covers):
    w = (mass_density - rho pi/4 d^2) g, EA = stiffness, in the order of the ``lines`` list.  Returns (records, depth)."""
    moor = design.get("mooring") if isinstance(design, dict) else None
    if not isinstance(moor, dict):
        raise UnsupportedFOWT("the design has no mooring section")
    if "file" in moor:
        raise UnsupportedFOWT("the mooring system is a MoorDyn file (%s): only the YAML section is parsed" % moor["file"])
    if int(moor.get("moorMod", 0)) != 0:
        raise UnsupportedFOWT("moorMod = %s: line dynamics are not covered (moorMod 0 only)" % moor.get("moorMod"))
    depth = float(moor["water_depth"])
    points, types = {}, {}
    for p in moor.get("points", []):
        kind = str(p.get("type", "")).lower()
        if kind not in ("fixed", "vessel"):
            raise UnsupportedFOWT("mooring point %r is of type %r: free points are not covered" % (p.get("name"), p.get("type")))
        points[p["name"]] = (kind, np.array(p["location"], dtype=float).reshape(3))
    for t in moor.get("line_types", []):
        types[t["name"]] = t
    used = {}
    recs = []
    for ln in moor.get("lines", []):
        for end in ("endA", "endB"):
            if ln[end] not in points:
                raise UnsupportedFOWT("mooring line %r: unknown point %r" % (ln.get("name"), ln[end]))
            used[ln[end]] = used.get(ln[end], 0) + 1
        (kA, pA), (kB, pB) = points[ln["endA"]], points[ln["endB"]]
        if kA == "vessel" and kB == "vessel":
            raise UnsupportedFOWT("mooring line %r has both ends on the vessel" % ln.get("name"))
        if not (kA == "fixed" and kB == "vessel"):
            raise UnsupportedFOWT("mooring line %r must run from a fixed point (end A) to a vessel point (end B)" % ln.get("name"))
        if ln["type"] not in types:
            raise UnsupportedFOWT("mooring line %r: unknown line type %r" % (ln.get("name"), ln["type"]))
        t = types[ln["type"]]
        d = float(t["diameter"])
        rec = np.zeros(ML_N)
        rec[ML_ANCHOR:ML_ANCHOR + 3] = pA
        rec[ML_FAIRLEAD:ML_FAIRLEAD + 3] = pB
        rec[ML_L] = float(ln["length"])
        rec[ML_EA] = float(t["stiffness"])
        rec[ML_W] = (float(t["mass_density"]) - rho * (np.pi / 4 * d * d)) * g
        recs.append(rec)
    if not recs:
        raise UnsupportedFOWT("the mooring section has no lines")
    shared = [n for n, k in used.items() if k > 1]
    if shared:
        raise UnsupportedFOWT("mooring point %r joins %d lines: multi-segment and bridle layouts are not covered" % (shared[0], used[shared[0]]))
    return np.ascontiguousarray(recs), depth


def chains_from_design(design, rho=1025.0, g=9.81):
    """Row records [nRow,16] of ``design['mooring']`` with COMPOSITE lines: segments joined at ``free`` (or ``connection``)
    points that exactly two lines meet at, followed from each ``fixed`` point to a ``vessel`` point.  A line's rows are
    consecutive, anchor -> fairlead: the head row as in ``lines_from_design`` with the anchor-side segment's L, EA, w, then
    a continuation row per further segment (field 15 = 1, its own L, EA, w, and in field 10 the net submerged weight
    (m - rho v) g of the point at its lower end).  Lines come in the order of the ``lines`` list's anchor-side segments.
    Returns (records, depth, row_names); for a deck without free points the records are those of ``lines_from_design``."""
    moor = design.get("mooring") if isinstance(design, dict) else None
    if not isinstance(moor, dict):
        raise UnsupportedFOWT("the design has no mooring section")
    if "file" in moor:
        raise UnsupportedFOWT("the mooring system is a MoorDyn file (%s): only the YAML section is parsed" % moor["file"])
    if int(moor.get("moorMod", 0)) != 0:
        raise UnsupportedFOWT("moorMod = %s: line dynamics are not covered (moorMod 0 only)" % moor.get("moorMod"))
    depth = float(moor["water_depth"])
    points = {}
    for p in moor.get("points", []):
        kind = str(p.get("type", "")).lower()
        kind = "free" if kind == "connection" else kind
        if kind not in ("fixed", "vessel", "free"):
            raise UnsupportedFOWT("mooring point %r is of type %r" % (p.get("name"), p.get("type")))
        weight = (float(p.get("m", 0.0)) - rho * float(p.get("v", 0.0))) * g
        points[p["name"]] = (kind, np.array(p["location"], dtype=float).reshape(3), weight)
    types = {t["name"]: t for t in moor.get("line_types", [])}
    lines = list(moor.get("lines", []))
    if not lines:
        raise UnsupportedFOWT("the mooring section has no lines")
    at = {}                                                      # point -> the lines that end there
    for i, ln in enumerate(lines):
        for end in ("endA", "endB"):
            if ln[end] not in points:
                raise UnsupportedFOWT("mooring line %r: unknown point %r" % (ln.get("name"), ln[end]))
            at.setdefault(ln[end], []).append(i)
        if ln["type"] not in types:
            raise UnsupportedFOWT("mooring line %r: unknown line type %r" % (ln.get("name"), ln["type"]))
        if points[ln["endA"]][0] == "vessel" and points[ln["endB"]][0] == "vessel":
            raise UnsupportedFOWT("mooring line %r has both ends on the vessel" % ln.get("name"))
    for name, (kind, _, _) in points.items():
        k = len(at.get(name, []))
        if k > 2 or (k == 2 and kind != "free"):
            raise UnsupportedFOWT("mooring point %r joins %d lines: bridles and shared anchors or fairleads are not covered" % (name, k))
        if kind == "free" and k == 1:
            raise UnsupportedFOWT("free mooring point %r ends a single line: a dangling end is not covered" % name)

    def other(ln, name):
        return ln["endB"] if ln["endA"] == name else ln["endA"]

    recs, names, used = [], [], set()
    for i, ln in enumerate(lines):
        ends = [e for e in ("endA", "endB") if points[ln[e]][0] == "fixed"]
        if not ends or i in used:
            continue
        if len(ends) == 2:
            raise UnsupportedFOWT("mooring line %r runs between two fixed points" % ln.get("name"))
        here, rows, cur = ln[ends[0]], 0, i
        anchor = points[here][1]
        first = len(recs)
        while True:
            seg = lines[cur]
            used.add(cur)
            t = types[seg["type"]]
            d = float(t["diameter"])
            rec = np.zeros(ML_N)
            rec[ML_L] = float(seg["length"])
            rec[ML_EA] = float(t["stiffness"])
            rec[ML_W] = (float(t["mass_density"]) - rho * (np.pi / 4 * d * d)) * g
            if rows:
                rec[ML_WJOINT], rec[ML_CONT] = points[here][2], 1.0
            recs.append(rec)
            names.append(seg.get("name", "line%d" % (cur + 1)))
            rows += 1
            if rows > MAX_SEG:
                raise UnsupportedFOWT("the mooring line from %r has more than %d segments" % (ln[ends[0]], MAX_SEG))
            here = other(seg, here)
            kind = points[here][0]
            if kind == "vessel":
                break
            if kind == "fixed":
                raise UnsupportedFOWT("the mooring line from %r ends at the fixed point %r" % (ln[ends[0]], here))
            cur = [j for j in at[here] if j != cur][0]
        recs[first][ML_ANCHOR:ML_ANCHOR + 3] = anchor
        recs[first][ML_FAIRLEAD:ML_FAIRLEAD + 3] = points[here][1]
    left = [lines[j].get("name", "line%d" % (j + 1)) for j in range(len(lines)) if j not in used]
    if left:
        raise UnsupportedFOWT("mooring line %r belongs to a chain without a fixed end" % left[0])
    return np.ascontiguousarray(recs), depth, names


def bridles_from_design(design, rho=1025.0, g=9.81):
    """Row records [nRow,16] of ``design['mooring']`` with composite lines AND bridles: what ``chains_from_design`` accepts, plus
    ``free`` (or ``connection``) points of degree 3 .. MAX_LEG + 1 that have exactly one path to a ``fixed`` point -- the stem,
    through free points of degree 2 -- and direct lines to ``vessel`` points, the legs.  A bridle's rows are consecutive: the
    stem's rows as a composite line's (anchor -> junction, the head row's fairlead zero), then a leg row per leg (field 14 = 1,
    its fairlead in fields 3-5, its own L, EA, w; the junction's net submerged weight (m - rho v) g in field 10 of the first leg
    row), legs in the order of the ``lines`` list.  Lines and bridles come in the order of the list's anchor-side segments.
    Returns (records, depth, row_names); for a deck without bridles the records are those of ``chains_from_design``."""
    moor = design.get("mooring") if isinstance(design, dict) else None
    if not isinstance(moor, dict):
        raise UnsupportedFOWT("the design has no mooring section")
    if "file" in moor:
        raise UnsupportedFOWT("the mooring system is a MoorDyn file (%s): only the YAML section is parsed" % moor["file"])
    if int(moor.get("moorMod", 0)) != 0:
        raise UnsupportedFOWT("moorMod = %s: line dynamics are not covered (moorMod 0 only)" % moor.get("moorMod"))
    depth = float(moor["water_depth"])
    points = {}
    for p in moor.get("points", []):
        kind = str(p.get("type", "")).lower()
        kind = "free" if kind == "connection" else kind
        if kind not in ("fixed", "vessel", "free"):
            raise UnsupportedFOWT("mooring point %r is of type %r" % (p.get("name"), p.get("type")))
        weight = (float(p.get("m", 0.0)) - rho * float(p.get("v", 0.0))) * g
        points[p["name"]] = (kind, np.array(p["location"], dtype=float).reshape(3), weight)
    types = {t["name"]: t for t in moor.get("line_types", [])}
    lines = list(moor.get("lines", []))
    if not lines:
        raise UnsupportedFOWT("the mooring section has no lines")
    at = {}                                                      # point -> the lines that end there
    for i, ln in enumerate(lines):
        for end in ("endA", "endB"):
            if ln[end] not in points:
                raise UnsupportedFOWT("mooring line %r: unknown point %r" % (ln.get("name"), ln[end]))
            at.setdefault(ln[end], []).append(i)
        if ln["type"] not in types:
            raise UnsupportedFOWT("mooring line %r: unknown line type %r" % (ln.get("name"), ln["type"]))
        if points[ln["endA"]][0] == "vessel" and points[ln["endB"]][0] == "vessel":
            raise UnsupportedFOWT("mooring line %r has both ends on the vessel" % ln.get("name"))

    def other(ln, name):
        return ln["endB"] if ln["endA"] == name else ln["endA"]

    for name, (kind, _, _) in points.items():
        k = len(at.get(name, []))
        if kind != "free" and k > 1:
            raise UnsupportedFOWT("%s mooring point %r joins %d lines: shared anchors and fairleads are not covered" % (kind, name, k))
        if kind == "free" and k == 1:
            raise UnsupportedFOWT("free mooring point %r ends a single line: a dangling end is not covered" % name)
        if kind == "free" and k > MAX_LEG + 1:
            raise UnsupportedFOWT("free mooring point %r joins %d lines: a bridle has at most %d legs" % (name, k, MAX_LEG))
        if kind == "free" and k > 2:                              # a junction: one line towards the anchor, the others straight to the vessel
            far = [points[other(lines[j], name)][0] for j in at[name]]
            if far.count("vessel") != k - 1:
                what = [other(lines[j], name) for j in at[name] if points[other(lines[j], name)][0] != "vessel"]
                if any(points[q][0] == "free" and len(at[q]) > 2 for q in what):
                    raise UnsupportedFOWT("the junction %r is joined to another junction: not covered" % name)
                raise UnsupportedFOWT("the junction %r has %d lines that do not end on the vessel: a bridle has one stem, and its legs "
                                      "run straight to vessel points" % (name, len(what)))

    def record(seg):
        t = types[seg["type"]]
        d = float(t["diameter"])
        rec = np.zeros(ML_N)
        rec[ML_L] = float(seg["length"])
        rec[ML_EA] = float(t["stiffness"])
        rec[ML_W] = (float(t["mass_density"]) - rho * (np.pi / 4 * d * d)) * g
        return rec

    recs, names, used = [], [], set()
    for i, ln in enumerate(lines):
        ends = [e for e in ("endA", "endB") if points[ln[e]][0] == "fixed"]
        if not ends or i in used:
            continue
        if len(ends) == 2:
            raise UnsupportedFOWT("mooring line %r runs between two fixed points" % ln.get("name"))
        here, rows, cur = ln[ends[0]], 0, i
        anchor = points[here][1]
        first = len(recs)
        while True:
            seg = lines[cur]
            used.add(cur)
            rec = record(seg)
            if rows:
                rec[ML_WJOINT], rec[ML_CONT] = points[here][2], 1.0
            recs.append(rec)
            names.append(seg.get("name", "line%d" % (cur + 1)))
            rows += 1
            if rows > MAX_SEG:
                raise UnsupportedFOWT("the mooring line from %r has more than %d segments" % (ln[ends[0]], MAX_SEG))
            here = other(seg, here)
            kind = points[here][0]
            if kind == "vessel":
                recs[first][ML_FAIRLEAD:ML_FAIRLEAD + 3] = points[here][1]
                break
            if kind == "fixed":
                raise UnsupportedFOWT("the mooring line from %r ends at the fixed point %r" % (ln[ends[0]], here))
            nxt = [j for j in at[here] if j != cur]
            if len(nxt) > 1:                                     # the junction: the legs, in the order of the list
                for n, j in enumerate(sorted(nxt)):
                    used.add(j)
                    rec = record(lines[j])
                    rec[ML_FAIRLEAD:ML_FAIRLEAD + 3] = points[other(lines[j], here)][1]
                    rec[ML_LEG] = 1.0
                    if n == 0:
                        rec[ML_WJOINT] = points[here][2]
                    recs.append(rec)
                    names.append(lines[j].get("name", "line%d" % (j + 1)))
                break
            cur = nxt[0]
        recs[first][ML_ANCHOR:ML_ANCHOR + 3] = anchor
    left = [lines[j].get("name", "line%d" % (j + 1)) for j in range(len(lines)) if j not in used]
    if left:
        raise UnsupportedFOWT("mooring line %r belongs to a chain without a fixed end" % left[0])
    return np.ascontiguousarray(recs), depth, names


ML_UNIT_B, ML_UNIT_A = 11, 12  # array rows (include/raftx_array_mooring.h): the unit of end B; 0 or 1 + the unit of end A
ARRAY_MAX_UNIT = 6


def array_lines(unit_lines, locations, headings=None, shared=()):
    """Array rows [nRow,16] (include/raftx_array_mooring.h) of a farm: the records of every unit -- ``unit_lines`` [nUnit] of
    [nRow_i,16] from ``lines_from_design``, ``chains_from_design`` or ``bridles_from_design``, laid out about the origin --
    turned about the vertical by ``headings`` [nUnit] (degrees, counter-clockwise: heading_adjust of the deck's ``array:``
    table; anchors and fairleads turn together, the unit's pose stays unrotated as in the reference), their anchors shifted to
    ``locations`` [nUnit,2] (x_location, y_location) and stamped with the unit; then one shared row per entry of ``shared``:
    dicts unitA, rA, unitB, rB (unit indices and body-frame attachment points), L, EA, w.  The units' reference poses are
    (x_location, y_location, 0, 0, 0, 0)."""
    n_unit = len(unit_lines)
    if not 1 <= n_unit <= ARRAY_MAX_UNIT:
        raise ValueError("an array has 1 to %d units (got %d)" % (ARRAY_MAX_UNIT, n_unit))
    locations = np.asarray(locations, dtype=float).reshape(n_unit, 2)
    headings = np.zeros(n_unit) if headings is None else np.asarray(headings, dtype=float).reshape(n_unit)
    rows = []
    for u, recs in enumerate(unit_lines):
        recs = np.array(recs, dtype=float).reshape(-1, ML_N)
        if np.any(recs[:, ML_UNIT_B] != 0) or np.any(recs[:, ML_UNIT_A] != 0):
            raise ValueError("unit %d: the records carry unit fields already (fields 11-12 must be zero)" % u)
        c, s = np.cos(np.deg2rad(headings[u])), np.sin(np.deg2rad(headings[u]))
        if headings[u] % 90.0 == 0.0:                            # exact quarter turns
            c, s = np.round(c), np.round(s)
        for lo in (ML_ANCHOR, ML_FAIRLEAD):
            x, y = recs[:, lo].copy(), recs[:, lo + 1].copy()
            recs[:, lo], recs[:, lo + 1] = c * x - s * y, s * x + c * y
        head = (recs[:, ML_CONT] == 0) & (recs[:, ML_LEG] == 0)
        recs[head, ML_ANCHOR] += locations[u, 0]
        recs[head, ML_ANCHOR + 1] += locations[u, 1]
        recs[:, ML_UNIT_B] = u
        rows.append(recs)
    for k, sh in enumerate(shared):
        missing = [f for f in ("unitA", "rA", "unitB", "rB", "L", "EA", "w") if f not in sh]
        if missing:
            raise ValueError("shared line %d lacks %s" % (k, missing))
        ua, ub = sh["unitA"], sh["unitB"]
        for nm, v in (("unitA", ua), ("unitB", ub)):
            if int(v) != v or not 0 <= int(v) < n_unit:
                raise ValueError("shared line %d: %s = %r is no unit index 0 .. %d" % (k, nm, v, n_unit - 1))
        if int(ua) == int(ub):
            raise ValueError("shared line %d has both ends on unit %d" % (k, int(ua)))
        L, EA, w = float(sh["L"]), float(sh["EA"]), float(sh["w"])
        if not (L > 0 and EA > 0 and w > 0):
            raise ValueError("shared line %d: L, EA and w must be positive (got %g, %g, %g)" % (k, L, EA, w))
        rec = np.zeros(ML_N)
        rec[ML_ANCHOR:ML_ANCHOR + 3] = np.asarray(sh["rA"], dtype=float).reshape(3)
        rec[ML_FAIRLEAD:ML_FAIRLEAD + 3] = np.asarray(sh["rB"], dtype=float).reshape(3)
        rec[ML_L], rec[ML_EA], rec[ML_W] = L, EA, w
        rec[ML_UNIT_B], rec[ML_UNIT_A] = int(ub), int(ua) + 1
        rows.append(rec[None])
    if not rows or not sum(len(r) for r in rows):
        raise ValueError("the array has no rows")
    return np.ascontiguousarray(np.concatenate(rows))


def tension_names(n):
    """Names of the 2 n tension channels in the order of T / J: ends A of all lines, then ends B (getTensions)."""
    return ["Tmoor_A%d" % (i + 1) for i in range(n)] + ["Tmoor_B%d" % (i + 1) for i in range(n)]


class MooringProgram:
    """Edit program of the mooring lines of a parametric sweep (raftx_mooring_program): base records + anchor / fairlead
    coordinates that are affine in the sweep parameters -- value = c0 + c1*p1 + ..., left to right without fused
    multiply-adds, as ``VariantProgram.ends``."""

    def __init__(self, lines, n_param):
        self.lines = np.ascontiguousarray(lines, dtype=float).reshape(-1, ML_N).copy()
        self.n_param = int(n_param)
        n = len(self.lines)
        self.coef = np.zeros((n, 6, self.n_param + 1))
        self.edit = np.zeros(n, dtype=np.int32)

    @property
    def n(self):
        return len(self.lines)

    def ends(self, l, anchor, fairlead):
        """Anchor and fairlead of line l: [3][nParam+1] rows of coefficients each (constant, then one per parameter).
        Of a composite line they are the head row's: a continuation row is refused.  Of a bridle the head row has an anchor
        only and a leg row a fairlead only: the other argument must be None (or all zero)."""
        if self.lines[l, ML_CONT] != 0:
            raise ValueError("row %d is a continuation row of a composite line: its anchor and fairlead are the head row's" % l)
        shape = (3, self.n_param + 1)
        anchor = np.zeros(shape) if anchor is None else np.asarray(anchor, dtype=float).reshape(shape)
        fairlead = np.zeros(shape) if fairlead is None else np.asarray(fairlead, dtype=float).reshape(shape)
        if self.lines[l, ML_LEG] != 0 and np.any(anchor != 0):
            raise ValueError("row %d is a leg row of a bridle: it has a fairlead (fields 3-5) and no anchor" % l)
        if self.lines[l, ML_LEG] == 0 and self._heads_bridle(l) and np.any(fairlead != 0):
            raise ValueError("row %d heads a bridle: it has an anchor (fields 0-2) and no fairlead" % l)
        self.coef[l, :3] = anchor
        self.coef[l, 3:] = fairlead
        self.edit[l] = 1

    def _heads_bridle(self, l):
        k = l + 1
        while k < self.n and self.lines[k, ML_CONT] != 0:
            k += 1
        return k < self.n and self.lines[k, ML_LEG] != 0

    def expand(self, params):
        """The records [nD,nLine,16] of the variants ``params`` [nD,nParam] on the host: the library's evaluation order."""
        params = np.ascontiguousarray(params, dtype=float).reshape(-1, self.n_param)
        out = np.broadcast_to(self.lines, (len(params),) + self.lines.shape).copy()
        for l in np.flatnonzero(self.edit):
            for i in range(6):
                v = np.full(len(params), self.coef[l, i, 0])
                for q in range(self.n_param):
                    v = v + self.coef[l, i, 1 + q] * params[:, q]
                out[:, l, i] = v
        return out
