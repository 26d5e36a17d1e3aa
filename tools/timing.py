"""The timing scheme of the *_time.py tools and time_limit_bench.py, written once.

A tool's parent process never opens the GPU: it starts a fresh child per repeat (run_children), the child times its cases in an order that rotates with
the repeat (rotated) and prints them on one line (emit).  A case is timed with device events on the stream the work is issued on — the handle's own timer
(engine_timed) or torch events on torch's current stream (torch_timed) — after a warm-up, over a window sized from a short probe (window_of).  The parent
reduces each case's repeats to median, min, max and spread, (max - min) / median, the noise figure every comparison is read against (summarise), and
writes one record (write_record, write_json).  torch and numpy are imported where they are used, never at module level."""
import json
import statistics
import subprocess
import sys

RESULT = "RESULT "


def scaled(n, scale):
    """the population at --scale: whole multiples of 1024 environments, at least one"""
    return max(1024, int(n * scale)) // 1024 * 1024


def calibrate(timed, window_s, warm, probe):
    """warm-up, a probe of `probe` launches, and from it the number of launches that fill window_s seconds (at least the probe's)"""
    timed(warm)
    per = timed(probe) / probe                      # ms per launch
    return max(probe, int(window_s * 1000.0 / per) + 1)


def window_of(timed, window_s, warm, probe):
    """(ms, count) of the timed window; timed(count) launches count times and returns the milliseconds they took"""
    count = calibrate(timed, window_s, warm, probe)
    return timed(count), count


def engine_timed(env, launch):
    """timed(count) on the handle's own timer, the events on the stream its kernels run on"""
    def timed(count):
        env.timer_start()
        for _ in range(count):
            launch()
        ms = env.timer_stop()
        env.sync()                                  # (raises on a sticky device error)
        return ms
    return timed


def torch_timed(body, after=None):
    """timed(count) between two torch events on torch's current stream; `after` (a TorchVecEnv's check) runs once the window has drained"""
    import torch

    def timed(count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(count):
            body()
        e1.record()
        e1.synchronize()
        if after:
            after()
        return e0.elapsed_time(e1)
    return timed


def mlp_weights(D, A, H, in_scale=1.0):
    """nn.Linear-layout float32 weights (W1 [H, D], b1 [H], W2 [A, H], b2 [A]) of a one-hidden-layer policy: seeded normal draws, the first layer scaled to
    the observation's range (the timing depends on them only through how often episodes end)"""
    import numpy as np
    rng = np.random.default_rng(100 + H)
    return ((rng.normal(0, 1, (H, D)) * np.array(in_scale)).astype(np.float32), rng.normal(0, 0.5, H).astype(np.float32),
            (rng.normal(0, 1, (A, H)) / np.sqrt(H)).astype(np.float32), rng.normal(0, 0.1, A).astype(np.float32))


def torch_heads(sigma=None):
    """what turns the last layer's scores [n, A] into the actions TorchVecEnv.step takes, by the name mgym_rollout_mlp2 gives the head"""
    import torch
    return dict(greedy=lambda s: s.argmax(1).to(torch.int32),
                sample=lambda s: torch.multinomial(torch.softmax(s, 1), 1).squeeze(1).to(torch.int32),
                gauss=lambda s: s.squeeze(1) + sigma * torch.randn(s.shape[0], device=s.device, dtype=torch.float32))


def torch_policy_timed(env, weights, act, head, K):
    """timed(count) of the loop a trainer would run instead of a fused rollout, count * K steps on a TorchVecEnv with AoS observations: per step one
    torch.addmm per layer of `weights` (W1, b1, W2, b2, ...) with torch.relu / torch.tanh between them, head(scores), TorchVecEnv.step — eager kernels,
    the [n, H] activations through memory"""
    import torch
    w = [torch.from_numpy(x).cuda() for x in weights]
    layers = [(b, wt.t().contiguous()) for wt, b in zip(w[::2], w[1::2])]
    fn = torch.relu if act == "relu" else torch.tanh
    state = [env.reset()]

    def body():
        obs = state[0]
        for _ in range(K):
            h = obs
            for b, wt in layers[:-1]:
                h = fn(torch.addmm(b, h, wt))
            obs = env.step(head(torch.addmm(layers[-1][0], h, layers[-1][1])))[0]
        state[0] = obs
    return torch_timed(body, env.check)


def rotated(cases, rotate):
    """the cases from the rotate-th on, then the ones before it: no case keeps one place in the process over the repeats"""
    return cases[rotate % len(cases):] + cases[: rotate % len(cases)]


def emit(records):
    """a child's one line of results, for run_children to pick out of whatever else the child printed"""
    print(RESULT + json.dumps(records), flush=True)


def run_children(argv_of, labels, repeats, timeout, fields=lambda label, rep, position: dict(repeat=rep)):
    """Every repeat, one fresh python child per label, in order (labels: a list, or a function of the repeat that returns the list; [None] for a tool with
    one child per repeat): one process holds one case list or one build of the library, and the parent never opens the GPU.  argv_of(label, rep) is the
    child's command line after the interpreter.  Returns the children's records in the order they ran, each with fields(label, rep, position) added.
    A child that exits non-zero or prints no result line ends the run: the tails of its output go to stderr and SystemExit names it, so that nothing more
    is started on the GPU."""
    runs = []
    for rep in range(repeats):
        for position, label in enumerate(labels(rep) if callable(labels) else labels):
            who = "" if label is None else f" {label}"
            r = subprocess.run([sys.executable] + argv_of(label, rep), capture_output=True, text=True, timeout=timeout)
            line = [l for l in r.stdout.splitlines() if l.startswith(RESULT)]
            if r.returncode != 0 or not line:
                print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                raise SystemExit(f"worker{who} repeat {rep} failed with status {r.returncode}")
            runs += [dict(rec, **fields(label, rep, position)) for rec in json.loads(line[0][len(RESULT):])]
            print(f"repeat {rep}{who}: done", flush=True)
    return runs


def grouped(runs, key_of):
    """{key_of(record): [its ns_per_env_step over the repeats]}, in the order the records ran"""
    out = {}
    for rec in runs:
        out.setdefault(key_of(rec), []).append(rec["ns_per_env_step"])
    return out


def stats(v, repeats_as):
    """One summary row of a case's repeats (ns per env-step).  repeats_as "list": median, min, max, spread, env_steps_per_s, repeats = the values rounded
    to 6 places; "count": median, min, max, spread, repeats = how many, and the tool appends what else it reports.  The order of the fields is the
    committed records'."""
    med = statistics.median(v)
    row = dict(median=med, min=min(v), max=max(v), spread=(max(v) - min(v)) / med)
    if repeats_as == "list":
        row.update(env_steps_per_s=1e9 / med, repeats=[round(x, 6) for x in v])
    else:
        assert repeats_as == "count", repeats_as
        row.update(repeats=len(v))
    return row


def summarise(values_by_key, repeats_as):
    """{key: stats(values)} with the keys sorted"""
    return {k: stats(v, repeats_as) for k, v in sorted(values_by_key.items())}


median = statistics.median                         # (for the fields a tool reduces besides ns per env-step)


def write_record(path, head, table):
    """head fields, then "summary" with one line per case: the record stays readable in a diff"""
    with open(path, "w") as f:
        f.write("{\n")
        for k, v in head.items():
            f.write(f" {json.dumps(k)}: {json.dumps(v)},\n")
        f.write(' "summary": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in table.items()) + "\n }\n}\n")


def write_json(path, doc):
    """the whole document indented by one: the records that keep every run"""
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
