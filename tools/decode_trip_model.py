"""CPU model of the 8 bit packet loop of k_decode_blocks (hsrle_decode.hip.h, `S == 1`):  python tools/decode_trip_model.py [--waves N] [--seed S] [ORDER ...]
How often does a wave execute each SECTION of the loop per 128-byte step -- H (parse a header: lanes with lit == run == 0), L (copy literals), R (fill a run) --
when a trip of the loop runs the sections in a given ORDER (any sequence of the three letters: HLR is the loop as it was, LRH the rotation of dec8_loop_lrh,
LRHLR, RHLRH ... for what-ifs)?  64 lanes, one block of 4 KiB each; a step ends at a multiple of 128 OUTPUT bytes; a section counts once per trip as soon as one
lane of the wave needs it (the wave executes it for all); its chunk loop runs as long as the lane with the most 16-byte chunks (chunk iterations).  The ring is
taken as always resident (no stalls), a header as free of the block's end.

Packets as the two synthetic generators of the benchmark give them (tests/hsrle_testlib.py: synth_chunk_py), one (literals, run) pair per packet:
  runs   literals 1 .. 63, run 2 .. 63, both uniform                                       (run-distributed(8): the headline)
  video  1 .. 9 literals, run 40 .. 159 with probability 1/4, else 10 .. 25                   (video-shaped)
numpy only.  Prints, per generator and order: trips, H / L / R sections and literal / run chunk iterations per step.  tools/probe_kernel_stamps.py prints the
same three section counts as the kernel's stamp build counts them.

Lazy run fill (dec8_lazy_fill, hsrle_codecs.h): a second table counts the 16-byte LDS stores of the two copy sections.  Executed by the wave per step: literal chunk
iterations + run chunk iterations as the loop stands; with the lazy fill an R section executes ONE store, so the interior run chunk iterations (run chunk iterations
- R sections) go away.  Needed by a lane per step: its own literal and run chunks, and how many of its run chunks lie wholly inside the run behind the section's
first chunk -- the chunks a lazy kernel marks for the flush instead of storing them."""
import sys

import numpy as np

STEP, BLOCK, LANES = 128, 4096, 64


def packets(kind, rng, n, count):
    if kind == "runs":
        return rng.integers(1, 64, (n, count)), rng.integers(2, 64, (n, count))
    assert kind == "video"
    long_run = rng.integers(0, 4, (n, count)) == 0
    return rng.integers(1, 10, (n, count)), np.where(long_run, rng.integers(40, 160, (n, count)), rng.integers(10, 26, (n, count)))


def simulate(kind, order, waves=512, seed=1):
    rng = np.random.default_rng(seed)
    n = waves * LANES
    lits, runs = packets(kind, rng, n, BLOCK // 3)
    lane = np.arange(n)
    nxt = np.zeros(n, dtype=np.int64)
    lit, run, o = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    count = dict(trips=0, H=0, L=0, R=0, lit_chunks=0, run_chunks=0, lane_lit=0.0, lane_run=0.0, lane_lazy=0.0)
    per_wave = lambda m: m.reshape(waves, LANES)
    steps = BLOCK // STEP
    for s in range(steps):
        target = (s + 1) * STEP
        while True:
            act = o < target
            if not act.any():
                break
            count["trips"] += int(per_wave(act).any(1).sum())
            for sec in order:
                if sec == "H":
                    need = act & (lit == 0) & (run == 0) & (o < target)
                    lit[need], run[need] = lits[lane[need], nxt[need]], runs[lane[need], nxt[need]]
                    nxt[need] += 1
                elif sec == "L":
                    need = act & (lit > 0) & (o < target)
                    m = np.minimum(lit, target - o) * need
                    count["lit_chunks"] += int(per_wave(((o & 15) + m + 15) // 16 * need).max(1).sum())
                    count["lane_lit"] += float((((o & 15) + m + 15) // 16 * need).sum()) / LANES
                    o += m
                    lit -= m
                else:
                    need = act & (lit == 0) & (run > 0) & (o < target)
                    m = np.minimum(run, target - o) * need
                    count["run_chunks"] += int(per_wave(((o & 15) + m + 15) // 16 * need).max(1).sum())
                    count["lane_run"] += float((((o & 15) + m + 15) // 16 * need).sum()) / LANES
                    count["lane_lazy"] += float((np.maximum(((o & 15) + m) // 16 - 1, 0) * need).sum()) / LANES      # chunks wholly inside the run, behind the first
                    o += m
                    run -= m
                count[sec] += int(per_wave(need).any(1).sum())
    return {k: v / (waves * steps) for k, v in count.items()}


def main(argv):
    waves, seed, orders = 512, 1, []
    it = iter(argv)
    for a in it:
        if a == "--waves":
            waves = int(next(it))
        elif a == "--seed":
            seed = int(next(it))
        else:
            assert a and set(a) <= set("HLR"), "an order is a sequence of the letters H, L, R"
            orders.append(a)
    orders = orders or ["HLR", "RHL", "LRH"]
    print("| data | order | trips per step | H sections | L | R | literal chunk iterations | run chunk iterations |")
    print("|---|---|---:|---:|---:|---:|---:|---:|")
    results = [(kind, order, simulate(kind, order, waves, seed)) for kind in ("runs", "video") for order in orders]
    for kind, order, r in results:
        print("| %s | %s | %.2f | %.2f | %.2f | %.2f | %.1f | %.1f |" % (kind, " ".join(order), r["trips"], r["H"], r["L"], r["R"], r["lit_chunks"], r["run_chunks"]))
    print("\n| data | order | interior run chunk iterations | wide LDS stores executed per step | with the lazy fill | a lane needs: literal chunks | run chunks | of them marked, not stored |")
    print("|---|---|---:|---:|---:|---:|---:|---:|")
    for kind, order, r in results:
        print("| %s | %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f |" % (kind, " ".join(order), r["run_chunks"] - r["R"], r["lit_chunks"] + r["run_chunks"], r["lit_chunks"] + r["R"],
                                                                      r["lane_lit"], r["lane_run"], r["lane_lazy"]))


if __name__ == "__main__":
    main(sys.argv[1:])
