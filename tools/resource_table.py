"""Table of -Rpass-analysis=kernel-resource-usage remarks (hipcc's stderr on
stdin or in the files given): kernel, VGPRs, AGPRs, spills, occupancy, LDS.
    hipcc ... -Rpass-analysis=kernel-resource-usage -c x.hip 2>&1 | python tools/resource_table.py
"""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                             check=True).stdout.split("\n")
        out = [re.sub(r"pp2::\(anonymous namespace\)::|pp2::|^void ", "", o) for o in out]
        return [o[:o.index(">") + 1] if "<" in o.split("(")[0] else o.split("(")[0] for o in out]
    except (OSError, subprocess.CalledProcessError):
        return names


def main():
    text = "".join(open(f).read() for f in sys.argv[1:]) if len(sys.argv) > 1 else sys.stdin.read()
    rows, cur = [], None
    for line in text.split("\n"):
        m = re.search(r"remark: .*?(Function Name|VGPRs|AGPRs|SGPRs Spill|VGPRs Spill|"
                      r"Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|ScratchSize \[bytes/lane\]): (\S+)",
                      line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    names = demangle([r["name"] for r in rows])
    print(f"{'kernel':58s} {'VGPR':>5s} {'AGPR':>5s} {'Vspill':>6s} {'Sspill':>6s} {'scratch':>7s} {'occ':>4s}")
    for r, n in zip(rows, names):
        print(f"{n[:58]:58s} {r.get('VGPRs', '?'):>5s} {r.get('AGPRs', '?'):>5s} "
              f"{r.get('VGPRs Spill', '?'):>6s} {r.get('SGPRs Spill', '?'):>6s} "
              f"{r.get('ScratchSize [bytes/lane]', '?'):>7s} {r.get('Occupancy [waves/SIMD]', '?'):>4s}")


if __name__ == "__main__":
    main()
