"""Worker of tests/test_checkpoint_gpu.py's resume test: one PROCESS of a training run under opt.checkpoint.

    python _checkpoint_worker.py <root> <epochs> <resume: 0 | 1>

For each variant ("plain", "pruned": opt.prune_schedule = [(1, 0.5)]) a Main on <root>/<variant> runs <epochs> epochs of
data.synthetic_digits(600, 200), 784-32-24-10, batch 100, S = 2; with resume = 1 it starts from <root>/<variant>/model
(opt.network_to_load). The test compares the run directories; nothing of a run survives the process but its files."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vbnn_amd import data, train            # noqa: E402

VARIANTS = {"plain": {}, "pruned": {"prune_schedule": [(1, 0.5)]}}


def main():
    root, epochs, resume = sys.argv[1], int(sys.argv[2]), sys.argv[3] == "1"
    trainSet, testSet = data.synthetic_digits(600, 200)
    for name, over in VARIANTS.items():
        d = os.path.join(root, name)
        opt = train.default_opt(network_name=d, hidden=[32, 24], batchSize=100, testBatchSize=100, trainSize=600, testSize=200, S=2,
                                testSamples=2, state={"learningRate": 5e-2}, meanState={"learningRate": 2e-3},
                                varState={"learningRate": 5e-2}, checkpoint=True, **over)
        if resume:
            opt["network_to_load"] = d
        m = train.Main(opt)
        hist = m.run(trainSet, testSet, epochs=epochs)
        m.log.close()
        print(f"{name}: epoch {m.epoch}, draw {m.net.draw}, held {m.net.held}, devacc {hist[-1]['devacc']}", flush=True)


if __name__ == "__main__":
    main()
