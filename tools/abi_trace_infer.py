"""tools/abi_trace.py's recording proxy on the INFERENCE programs: one line per C-ABI call of RaftFlow.forward in eval mode (with and without a source cache
of the same batch, fp32 and bf16, corr="volume" and "direct") and of the Animator / make_animation / reconstruction loops with one driving frame per source.

    python tools/abi_trace_infer.py OUT.txt

Two commits whose traces are equal line for line hand the library the same calls, and their `result` lines say the outputs are bit-equal (on the emulator)."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _abi_trace():
    spec = importlib.util.spec_from_file_location("abi_trace", os.path.join(ROOT, "tools", "abi_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _result(T, lines, tag, outs):
    for i, t in enumerate(outs):
        lines.append(f"result {tag} out{i} {T._hash(t.detach().contiguous().data_ptr(), 4 * t.numel())}")


def programs(T, lines):
    from mrfa_amd.infer import Animator, make_animation, reconstruction
    from mrfa_amd.modules import RaftFlow
    from mrfa_amd.utils.prng import det_uniform
    from tests import cases
    from tests.test_bf16_cache import _dry_model
    from tests.test_oracle_golden import raft_inputs
    for prior_only in (False, True):
        rf = RaftFlow(**cases.raft_cfg(64, prior_only))
        rf.load_state_dict(cases.weights_for(rf.state_dict(), "rf"))
        rf.eval()
        ins = raft_inputs(64, 2, "g3/raft64")
        for corr in ("volume", "direct"):
            for cache in (None, torch.float32, torch.bfloat16):
                lines.append(f"# program RaftFlow eval prior_only={prior_only} corr={corr} cache={cache}")
                kw = {} if cache is None else {"source_cache": rf.encode_source(ins[0], ins[3], ins[4], feature_dtype=cache)}
                _result(T, lines, f"raft/{prior_only}/{corr}/{cache}", rf(*ins, corr=corr, **kw))
    m = _dry_model()
    src = det_uniform("trace/src", (2, 3, 64, 64), 0, 1)
    clip = torch.stack([det_uniform(f"trace/drv{t}", (2, 3, 64, 64), 0, 1) for t in range(2)], dim=2)
    for corr in ("volume", "direct"):
        for dtype in (torch.float32, torch.bfloat16):
            lines.append(f"# program Animator corr={corr} cache={dtype}")
            an = Animator(m, corr=corr, cache_dtype=dtype)
            an.set_source(src)
            _result(T, lines, f"animator/{corr}/{dtype}", [an(clip[:, :, t].contiguous()) for t in range(2)])
        lines.append(f"# program make_animation / reconstruction corr={corr}")
        _result(T, lines, f"make_animation/{corr}", [make_animation(m, src, clip, relative=True, adapt_movement_scale=True, corr=corr)])
        _result(T, lines, f"reconstruction/{corr}", [reconstruction(m, clip, corr=corr)["prediction"]])


def main(out_path):
    T = _abi_trace()
    lines = []
    with T.traced_hip(lines), torch.no_grad():
        programs(T, lines)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} lines -> {out_path}")


if __name__ == "__main__":
    main(sys.argv[1])
