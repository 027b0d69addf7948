"""Print, for one kernel of a -S listing, the order of buffer loads / stores, vmcnt waits, LDS reads and branches behind the last MFMA."""
import re, sys
path, pat = sys.argv[1], sys.argv[2]
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*:", l) and pat in l)
end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
body = lines[start:end]
last = max(i for i, l in enumerate(body) if "v_mfma" in l)
out = []
for l in body[last + 1:]:
    t = l.strip().split(";")[0].strip()
    if not t:
        continue
    if re.match(r"^\.LBB", t):
        out.append("|" + t.rstrip(":"))
        continue
    op = t.split()[0]
    if op.startswith("buffer_load_dwordx4"): out.append("L4")
    elif op.startswith("buffer_load_dword"): out.append("L1")
    elif op.startswith("global_load"): out.append("GL")
    elif op.startswith("buffer_store"): out.append("ST")
    elif op.startswith("global_store") : out.append("GS")
    elif op.startswith("scratch_"): out.append("SCRATCH")
    elif op == "s_waitcnt":
        m = re.search(r"vmcnt\((\d+)\)", t)
        if m: out.append("w%s" % m.group(1))
    elif op.startswith("ds_read_b128") or op.startswith("ds_read2_b64"): out.append("r")
    elif op.startswith("ds_write"): out.append(".")
    elif op.startswith("v_ldexp"): out.append("x")
    elif op.startswith("s_cbranch") or op == "s_branch": out.append("BR")
    elif op.startswith("s_barrier"): out.append("BAR")
s = " ".join(out)
s = re.sub(r"(?:\. )+", lambda m: "[%dw] " % (len(m.group(0)) // 2), s)
s = re.sub(r"(?:x )+", lambda m: "[%dx] " % (len(m.group(0)) // 2), s)
print(lines[start][:120])
print(s)
