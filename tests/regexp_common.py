"""Shared helpers of the REGEXP_LIKE / LIKE tests: the Python yardstick and seeded generators of subset patterns and
of values."""
import random
import re


def yardstick(pattern, value):
    """Matcher.find() of Pattern.compile(pattern, CASE_INSENSITIVE | UNICODE_CASE) as Python computes it:
    re.compile(pattern, re.IGNORECASE | re.ASCII).search(value).

    Valid ONLY for patterns inside the accepted subset (include/pinotgpu.h, PGPU_PRED_REGEXP_LIKE) and for ASCII values
    without \\n or \\r: there the two engines mean the same language ('.' and '$' differ on line terminators, the
    case folding differs beyond ASCII, and many constructs outside the subset differ in syntax or meaning)."""
    return _compiled(pattern).search(value) is not None


_cache = {}


def _compiled(pattern):
    c = _cache.get(pattern)
    if c is None:
        if len(_cache) > 4096:
            _cache.clear()
        c = _cache[pattern] = re.compile(pattern, re.IGNORECASE | re.ASCII)
    return c


ALPHABET = "abAB01_-. /"      # values: small, so that matches are common
_LITERALS = "abAB01_ /"       # pattern literals that need no escape
_ESCAPED = ".-+*?()[]{}|^$\\<>&/"


def random_value(rng, max_len=10):
    return "".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, max_len)))


def random_values(seed, n, max_len=10):
    rng = random.Random(seed)
    return [random_value(rng, max_len) for _ in range(n)]


def _class(rng):
    items = []
    neg = rng.random() < 0.3
    if rng.random() < 0.15:
        items.append("-")
    for _ in range(rng.randint(1, 3)):
        k = rng.random()
        if k < 0.4:
            items.append(rng.choice("abAB01_ ./"))
        elif k < 0.6:
            lo, hi = sorted(rng.sample("abcd", 2))
            items.append("%s-%s" % (lo, hi) if rng.random() < 0.5 else "%s-%s" % (lo.upper(), hi.upper()))
        elif k < 0.7:
            items.append("0-%s" % rng.choice("19"))
        elif k < 0.85:
            items.append("\\" + rng.choice("dwsDWS"))
        else:
            items.append("\\" + rng.choice("-.]^\\["))
    if rng.random() < 0.15:
        items.append("^")       # a literal: never first
    if rng.random() < 0.15:
        items.append("-")       # a literal: last
    body = "".join(items)
    if body.startswith("^") and not neg:
        body = "a" + body
    return "[" + ("^" if neg else "") + body + "]"


def _atom(rng, depth, budget):
    k = rng.random()
    if depth < 3 and budget[0] > 2 and k < 0.2:
        inner = _alt(rng, depth + 1, budget)
        return ("(?:" if rng.random() < 0.3 else "(") + inner + ")", True
    budget[0] -= 1
    if k < 0.55:
        return rng.choice(_LITERALS), True
    if k < 0.65:
        return ".", True
    if k < 0.78:
        return _class(rng), True
    if k < 0.86:
        return "\\" + rng.choice("dwsDWS"), True
    if k < 0.92:
        return "\\" + rng.choice(_ESCAPED), True
    if k < 0.96:
        return "^", False
    return "$", False


def _quantifier(rng):
    k = rng.random()
    if k < 0.25:
        return "*"
    if k < 0.45:
        return "+"
    if k < 0.65:
        return "?"
    lo = rng.randint(0, 3)
    if k < 0.78:
        return "{%d}" % lo
    if k < 0.88:
        return "{%d,}" % lo
    return "{%d,%d}" % (lo, rng.randint(lo, 4))


def _cat(rng, depth, budget):
    out = []
    for _ in range(rng.randint(0 if depth else 1, 4)):
        if budget[0] <= 0:
            break
        a, quantifiable = _atom(rng, depth, budget)
        if quantifiable and rng.random() < 0.3:
            a += _quantifier(rng)
        out.append(a)
    return "".join(out)


def _alt(rng, depth, budget):
    return "|".join(_cat(rng, depth, budget) for _ in range(1 if rng.random() < 0.7 else rng.randint(2, 3)))


def random_pattern(rng):
    """A pattern of the accepted subset: depth <= 3, <= 12 atoms, repeat bounds <= 4."""
    return _alt(rng, 0, [12])


def random_patterns(seed, n):
    rng = random.Random(seed)
    return [random_pattern(rng) for _ in range(n)]
