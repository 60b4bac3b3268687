"""SAM flag masks as the pileup calls and ``pileup_main`` take them: an int, or a string that is decimal, ``0x`` hex
or a comma list of samtools' flag names. No GPU and no library: the CLI validates its options through this before
torch is imported."""
from __future__ import annotations

FLAG_NAMES = {"PAIRED": 0x1, "PROPER_PAIR": 0x2, "UNMAP": 0x4, "MUNMAP": 0x8, "REVERSE": 0x10, "MREVERSE": 0x20,
              "READ1": 0x40, "READ2": 0x80, "SECONDARY": 0x100, "QCFAIL": 0x200, "DUP": 0x400,
              "SUPPLEMENTARY": 0x800}
MAX_FLAGS = 0xFFFF


def parse_flags(value, what: str = "flags") -> int:
    """-> the mask 0..0xFFFF of ``value``; ValueError naming ``what`` for anything else. None is 0."""
    if value is None:
        return 0
    if isinstance(value, bool):
        raise ValueError("%s: expected a flag mask, got %r" % (what, value))
    if isinstance(value, int):
        mask = value
    else:
        text = str(value).strip()
        if not text:
            raise ValueError("%s: an empty flag mask" % what)
        low = text.lower()
        if low.startswith("0x") and all(c in "0123456789abcdef" for c in low[2:]) and len(low) > 2:
            mask = int(low, 16)
        elif text.isascii() and text.isdigit():
            mask = int(text)
        else:
            mask = 0
            for name in text.split(","):
                key = name.strip().upper()
                if key not in FLAG_NAMES:
                    raise ValueError("%s: unknown flag %r; known: %s, a decimal or a 0x hex mask"
                                     % (what, name.strip(), ", ".join(FLAG_NAMES)))
                mask |= FLAG_NAMES[key]
    if mask < 0 or mask > MAX_FLAGS:
        raise ValueError("%s: %r is outside 0..0xFFFF" % (what, value))
    return mask


def parse_filter(require, exclude):
    """-> (require mask, exclude mask); ValueError when one does not parse or they share a bit (no record passes)."""
    rq, ex = parse_flags(require, "require_flags"), parse_flags(exclude, "exclude_flags")
    if rq & ex:
        raise ValueError("require_flags 0x%x and exclude_flags 0x%x share bits 0x%x: no record could pass"
                         % (rq, ex, rq & ex))
    return rq, ex
