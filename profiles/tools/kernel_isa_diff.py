#!/usr/bin/env python3
"""Compare two device assembly files (hipcc --cuda-device-only -S) kernel by kernel.

    kernel_isa_diff.py BEFORE.s AFTER.s [--stats SUBSTRING]

A kernel body runs from its symbol line (`_Z...k_...:`) to its `.Lfunc_end` label: instructions and kernel
descriptor.  Prints one line per kernel that is missing, added or different, then a summary; with --stats, the
resource figures and a few instruction counts of every kernel whose (mangled) name contains SUBSTRING, before
and after.  Exit status 0 if every kernel present in both files is textually identical, else 1.
"""
import re
import sys

SYMBOL = re.compile(r"^(_Z\w*k_\w+):")
RESOURCES = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size", ".amdhsa_private_segment_fixed_size")
COUNTED = ("v_mad_u64_u32", "ds_read_b128", "ds_read2_b64", "s_waitcnt")


def kernels(path):
    """name -> (body text, resource directives of its .amdhsa_kernel block)"""
    bodies, res, name, lines, desc = {}, {}, None, [], None
    with open(path) as f:
        for line in f:
            m = SYMBOL.match(line)
            if m and name is None:
                name, lines = m.group(1), []
            if name is not None:
                lines.append(line)
                if line.startswith(".Lfunc_end"):
                    # local labels carry the function's ordinal in the file (.LBB35_8, .Lfunc_end35): not part of the kernel
                    n = line[len(".Lfunc_end"):].rstrip(":\n")
                    bodies[name] = re.sub(r"(\.L[A-Za-z_]+)" + n + r"(?!\d)", r"\1", "".join(lines))
                    name = None
            s = line.split()  # (the kernel descriptor sits inside the body, ahead of .Lfunc_end)
            if len(s) == 2 and s[0] == ".amdhsa_kernel":
                desc = s[1]
                res[desc] = {}
            elif desc and s and s[0] == ".end_amdhsa_kernel":
                desc = None
            elif desc and len(s) == 2 and s[0] in RESOURCES:
                res[desc][s[0]] = s[1]
    return bodies, res


def stats(body, res):
    out = [f"{k.replace('.amdhsa_', '')}={res.get(k, '?')}" for k in RESOURCES]
    for op in COUNTED:
        n = len(re.findall(r"^\s+" + op + r"\b", body, re.M))
        out.append(f"{op}={n}")
    return " ".join(out)


def main(argv):
    if len(argv) not in (3, 5) or (len(argv) == 5 and argv[3] != "--stats"):
        sys.exit(__doc__)
    (b0, r0), (b1, r1) = kernels(argv[1]), kernels(argv[2])
    same = [k for k in b0 if k in b1 and b0[k] == b1[k]]
    differ = [k for k in b0 if k in b1 and b0[k] != b1[k]]
    gone = [k for k in b0 if k not in b1]
    new = [k for k in b1 if k not in b0]
    for tag, names in (("DIFFERENT", differ), ("GONE", gone), ("NEW", new)):
        for k in names:
            print(f"{tag} {k}")
    print(f"{len(b0)} kernels before, {len(b1)} after: {len(same)} identical, {len(differ)} different, {len(gone)} gone, {len(new)} new")
    if len(argv) == 5:
        for tag, b, r in (("before", b0, r0), ("after ", b1, r1)):
            for k in b:
                if argv[4] in k:
                    print(f"{tag} {k}: {stats(b[k], r.get(k, {}))}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
