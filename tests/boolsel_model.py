"""numpy model of the Boolean line query semantics (include/ugpu.h,
ugpu_select_lines_bool), built on linesel_model; shared by
tests/test_boolsel_host.py and tests/test_boolsel.py."""
import numpy as np

import linesel_model as M


def literals(data, lists):
    """bool[nlists][nlines]: list t touches line k.  lists: (starts, lens or None)."""
    nlines = M.line_table(data)[0].size
    out = np.zeros((len(lists), nlines), bool)
    for t, (starts, lens) in enumerate(lists):
        out[t] = M.touched(data, starts, lens)
    return out


def formula(bits, clauses):
    """The AND over the clauses (pos, neg) of: some pos literal true or some
    neg literal false.  bits: bool[nlists][...]; no clause: true everywhere."""
    acc = np.ones(bits.shape[1:], bool)
    for pos, neg in clauses:
        hold = np.zeros(bits.shape[1:], bool)
        for t in range(bits.shape[0]):
            if pos >> t & 1:
                hold |= bits[t]
            if neg >> t & 1:
                hold |= ~bits[t]
        acc &= hold
    return acc


def select(data, lists, clauses, invert=False, files=False):
    """(begin, end, lineno) uint64 arrays of the selected lines, the line count
    and `whole`.  files: the literals are taken over the whole input (list t
    touches any line); when the formula holds the lines any list touches are
    selected, else none; invert complements the selection per line."""
    begin, end = M.line_table(data)
    lit = literals(data, lists)
    if files:
        whole = bool(formula(lit.any(axis=1).reshape(-1, 1), clauses)[0])
        pick = lit.any(axis=0) if whole else np.zeros(len(begin), bool)
    else:
        pick = formula(lit, clauses)
        whole = None
    if invert:
        pick = ~pick
    if whole is None:
        whole = bool(pick.any())
    sel = np.flatnonzero(pick)
    return begin[sel].astype(np.uint64), end[sel].astype(np.uint64), (sel + 1).astype(np.uint64), len(begin), whole


def grep(data, lists, clauses, invert=False, files=False, before=0, after=0):
    """[(lineno, kind)] the CLI prints, from the model alone.  Without a
    pattern the reference's primary pattern is empty and matches every line,
    with --files too (grep_bool)."""
    _, _, sel, nlines, _ = select(data, lists, clauses, invert, files and len(lists) > 0)
    lineno, kind = M.context_sets(sel, nlines, before, after)
    return [list(x) for x in zip(lineno, kind)]
