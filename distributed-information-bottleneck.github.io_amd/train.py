"""`python -m dib_amd.train` - the reference's `train.py` Keras path on the MI355X-native engine.

Mirrors reference train.py:12-178 (same flag names and defaults; the argparse `type=bool` trap and the
`infonce_space_dimensionality` typo of the reference are fixed): dataset dict ->
DistributedIBNet -> compile -> callbacks -> fit -> History post-processing (beta / KL in bits / loss without
the KL term) -> distributed information plane PNG.  `--infonce_loss True` runs the InfoNCE custom loop
(train.py:180-289, infonce.fit_infonce).  Both paths save the compression matrices every
`--save_compression_matrices_frequency` epochs (train.py:163-166, 251-261): feature by feature or, with
`--compression_matrices_one_launch True`, all features from one evaluation.

Multi-GPU: launch with `python -m torch.distributed.run --nproc-per-node N -m dib_amd.train ...`; every rank
runs the same script, gradients are all-reduced over RCCL.
"""
from __future__ import annotations

import argparse
import os

import numpy as np


def _bool(v):
    if isinstance(v, bool):
        return v
    return str(v).lower() in ("1", "true", "yes", "y", "t")


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Distributed IB training (MI355X-native)")
    p.add_argument('--dataset', default='boolean_circuit', choices=['boolean_circuit', 'synthetic_tabular', 'double_pendulum', 'table'])
    p.add_argument('--data_path', type=str, default='./data/')
    p.add_argument('--artifact_outdir', type=str, default='./training_artifacts/')
    p.add_argument('--ib', type=_bool, default=False, help='vanilla IB: treat all features as one (train.py:111-113)')
    p.add_argument('--learning_rate', type=float, default=3e-4)
    p.add_argument('--beta_start', type=float, default=1e-4)
    p.add_argument('--beta_end', type=float, default=3e0)
    p.add_argument('--number_pretraining_epochs', type=int, default=10 ** 3)
    p.add_argument('--number_annealing_epochs', type=int, default=10 ** 4)
    p.add_argument('--batch_size', type=int, default=128)
    p.add_argument('--use_positional_encoding', type=_bool, default=True)
    p.add_argument('--activation_fn', type=str, default='relu')
    p.add_argument('--feature_embedding_dimension', type=int, default=32)
    p.add_argument('--optimizer', type=str, default='adam',
                   help='a Keras optimizer name: adam, sgd, rmsprop, adagrad, adadelta, adamax, nadam (Keras defaults)')
    p.add_argument('--clipnorm', type=float, default=None, help='clip every variable\'s gradient to this L2 norm (Keras clipnorm)')
    p.add_argument('--clipvalue', type=float, default=None, help='clip every gradient element to [-v, v] (Keras clipvalue)')
    p.add_argument('--global_clipnorm', type=float, default=None,
                   help='clip the gradient of all variables to this joint L2 norm (Keras global_clipnorm)')
    p.add_argument('--learning_rate_decay', type=float, default=None,
                   help='legacy Keras `decay`: learning_rate / (1 + decay * iterations)')
    p.add_argument('--save_compression_matrices_frequency', type=int, default=0)
    p.add_argument('--compression_matrices_one_launch', type=_bool, default=False,
                   help='evaluate the compression matrices of all features from one encoder-bank forward and one launch per '
                        'save instead of feature by feature')
    p.add_argument('--info_bounds_frequency', type=int, default=0,
                   help='every N epochs: InfoNCE / leave-one-out bounds of every feature on the validation inputs '
                        '(info_bounds.npz + distributed_info_plane_mi.png in --artifact_outdir); 0 = off')
    p.add_argument('--feature_encoder_architecture', type=int, nargs='+', default=[128, 128])
    p.add_argument('--number_positional_encoding_frequencies', type=int, default=5)
    p.add_argument('--integration_network_architecture', type=int, nargs='+', default=[256, 256])
    p.add_argument('--infonce_loss', type=_bool, default=False)
    p.add_argument('--infonce_shared_dimensionality', type=int, default=64)
    p.add_argument('--infonce_y_encoder_architecture', type=int, nargs='+', default=[128, 128])
    p.add_argument('--infonce_similarity', type=str, default='l2')
    p.add_argument('--infonce_temperature', type=float, default=1.)
    p.add_argument('--pendulum_time_delta', type=float, default=2)
    p.add_argument('--pendulum_number_trajectories', type=int, default=0, help='0 = simulator default (1000)')
    p.add_argument('--boolean_random_circuit', type=_bool, default=False)
    p.add_argument('--boolean_number_input_gates', type=int, default=10)
    p.add_argument('--subset_information', type=_bool, default=False,
                   help='--dataset boolean_circuit: after fit, I(X_S;Y) of every subset of the input gates and their Shapley '
                        'values (subset_information.npz + subset_information.png in --artifact_outdir); at most 20 gates')
    p.add_argument('--synthetic_rows', type=int, default=1 << 20)
    p.add_argument('--synthetic_features', type=int, default=64)
    p.add_argument('--table_path', type=str, default=None,
                   help="--dataset table: an .npz with x, y and optional columns, or a .csv (data.fetch_table)")
    p.add_argument('--table_target', type=str, default=None, help='the target column (name or index) when it is part of the table; default the last')
    p.add_argument('--table_problem', type=str, default='classification', choices=['classification', 'regression'])
    p.add_argument('--table_categorical', type=str, nargs='*', default=[], help='names or indices of the columns to one-hot')
    p.add_argument('--table_quantile_noise', type=float, default=1e-3)
    p.add_argument('--table_n_quantiles', type=int, default=2000)
    p.add_argument('--table_valid_fraction', type=float, default=0.2)
    p.add_argument('--seed', type=int, default=0, help='noise / init / shuffle seed (the reference is unseeded)')
    p.add_argument('--verbose', type=_bool, default=False)
    p.add_argument('--repeats', type=int, default=1,
                   help='Keras path only: train this many replicas in lockstep (DistributedIBEnsemble) with seeds --seed + r; writes '
                        'history_replicas.npz and one information plane with the replicas overlaid (not a reference flag)')
    return p.parse_args(argv)


def postprocess_history(h, number_features, loss_is_info_based):
    """reference train.py:168-178: per-epoch series from `history.history` - the task loss without its beta * sum KL term, KL
    in bits, info-based losses in bits (same dtypes: float32 beta / loss series updated in place, float64 KL) - plus the
    validation series the reference forgot to build."""
    F = number_features
    beta_series = np.float32(h['beta'])
    kl_series = np.stack([h[f'KL{f}'] for f in range(F)], -1)
    loss_series = np.float32(h['loss'])
    loss_series_validation = np.float32(h['val_loss'])
    loss_series -= beta_series * np.sum(kl_series, axis=-1)
    kl_series /= np.log(2)
    kl_series_validation = np.stack([h[f'val_KL{f}'] for f in range(F)], -1)
    loss_series_validation -= np.float32(h['val_beta']) * np.sum(kl_series_validation, axis=-1)
    kl_series_validation /= np.log(2)
    if loss_is_info_based:
        loss_series /= np.log(2)
        loss_series_validation /= np.log(2)
    return dict(beta=beta_series, kl_bits=kl_series, loss=loss_series, kl_bits_validation=kl_series_validation,
                loss_validation=loss_series_validation)


def save_compression_matrices_npz(saver, outdir):
    """compression_matrices.npz of a SaveCompressionMatricesCallback: `epochs` and `beta` of its saves and one array
    `epoch{e}_feature{f}` per matrix."""
    epochs = sorted(saver.betas)
    np.savez(os.path.join(outdir, 'compression_matrices.npz'), epochs=np.int64(epochs),
             beta=np.float32([saver.betas[e] for e in epochs]),
             **{f'epoch{e}_feature{f}': m for (e, f), m in saver.matrices.items()})


def check_subset_information_args(args):
    """--subset_information goes with the Keras path on --dataset boolean_circuit and at most 20 input gates (2^20 subsets)"""
    if not args.subset_information:
        return
    from .subset_information import MAX_BITS
    if args.dataset != 'boolean_circuit' or args.infonce_loss:
        raise ValueError("--subset_information True goes with --dataset boolean_circuit (and not with --infonce_loss)")
    gates = args.boolean_number_input_gates if args.boolean_random_circuit else 10
    if gates > MAX_BITS:
        raise ValueError(f"--subset_information True: {gates} input gates have 2^{gates} subsets; the exhaustive table is "
                         f"limited to {MAX_BITS} gates")


def save_subset_information(dataset_dict, kl_series, loss_series, outdir, threshold=0.1):
    """the exhaustive I(X_S;Y) of the circuit's truth table next to what the fit kept: the subsets of gates whose KL stayed above
    `threshold` bits (circuit.selected_subsets) are the coloured points of the figure, the curve is (sum KL, H(Y) - loss)"""
    from . import circuit, subset_information
    info = subset_information.subset_information(dataset_dict['x_train'], dataset_dict['y_train'])
    selected = [list(map(int, s)) for s in circuit.selected_subsets(kl_series, threshold)]
    return subset_information.save_subset_information(
        info, outdir, selected=selected, info_in_full=np.sum(kl_series, axis=-1),
        predictive_information_out=info.entropy_y_bits - np.asarray(loss_series, dtype=np.float64), plot_start_ind=0)


def check_repeats_args(args):
    """--repeats N > 1 is the lockstep ensemble: the Keras path in one process, Adam at a constant rate, no per-epoch callbacks"""
    if args.repeats < 1:
        raise ValueError("--repeats must be at least 1")
    if args.repeats == 1:
        return
    if args.infonce_loss:
        raise ValueError("--repeats goes with the Keras path (not with --infonce_loss True)")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("--repeats trains all replicas in ONE process: run it without a multi-process launcher")
    if args.save_compression_matrices_frequency > 0 or args.info_bounds_frequency > 0 or args.subset_information:
        raise ValueError("--repeats: compression matrices, information bounds and the subset table are per-model callbacks; train "
                         "with --repeats 1, or take a replica out of the ensemble with to_model(r)")


def train_repeats(args, dataset_dict, optimizer, activation, number_epochs):
    """--repeats N: N replicas with seeds --seed + r in lockstep; history_replicas.npz holds, per replica, the post-processed
    series of postprocess_history (reference train.py:169-178), stacked on a leading replica axis"""
    from . import ensemble, visualization
    ens = ensemble.DistributedIBEnsemble(
        args.repeats, dataset_dict['feature_dimensionalities'], args.feature_encoder_architecture,
        args.integration_network_architecture, dataset_dict['output_dimensionality'],
        use_positional_encoding=args.use_positional_encoding,
        number_positional_encoding_frequencies=args.number_positional_encoding_frequencies, activation_fn=activation,
        feature_embedding_dimension=args.feature_embedding_dimension, output_activation_fn=dataset_dict['output_activation_fn'],
        noise_seed=args.seed, init_seed=args.seed, shuffle_seed=args.seed)
    ens.compile(optimizer=optimizer, loss=dataset_dict['loss'], metrics=dataset_dict['metrics'])
    histories = ens.fit(dataset_dict['x_train'], dataset_dict['y_train'], batch_size=args.batch_size, epochs=number_epochs,
                        validation_data=(dataset_dict['x_valid'], dataset_dict['y_valid']), shuffle=True,
                        beta_start=args.beta_start, beta_end=args.beta_end, number_pretraining_epochs=args.number_pretraining_epochs,
                        number_annealing_epochs=args.number_annealing_epochs, verbose=args.verbose)
    series = [postprocess_history(h.history, dataset_dict['number_features'], dataset_dict['loss_is_info_based']) for h in histories]
    stacked = {k: np.stack([s[k] for s in series]) for k in series[0]}
    print('Finished training.')
    np.savez(os.path.join(args.artifact_outdir, 'history_replicas.npz'), seeds=np.int64(ens.noise_seeds), **stacked)
    visualization.save_distributed_info_plane_replicas(stacked['kl_bits_validation'], stacked['loss_validation'], args.artifact_outdir)
    return histories


def main(argv=None):
    from . import data, models, optimizers, visualization
    args = get_args(argv)
    check_repeats_args(args)
    import torch
    import torch.distributed as dist
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl")
    rank = dist.get_rank() if dist.is_initialized() else 0
    number_epochs = args.number_pretraining_epochs + args.number_annealing_epochs
    check_subset_information_args(args)
    os.makedirs(args.artifact_outdir, exist_ok=True)
    dataset_dict = data.DATASETS[args.dataset](
        data_path=args.data_path, boolean_random_circuit=args.boolean_random_circuit,
        boolean_number_input_gates=args.boolean_number_input_gates, synthetic_rows=args.synthetic_rows,
        synthetic_features=args.synthetic_features, pendulum_time_delta=args.pendulum_time_delta,
        pendulum_number_trajectories=args.pendulum_number_trajectories, seed=args.seed, table_path=args.table_path,
        table_target=args.table_target, table_problem=args.table_problem, table_categorical=args.table_categorical,
        table_quantile_noise=args.table_quantile_noise, table_n_quantiles=args.table_n_quantiles,
        table_valid_fraction=args.table_valid_fraction)
    if dataset_dict['loss'] == 'infonce' and not args.infonce_loss:
        raise ValueError(f"dataset {args.dataset} trains with --infonce_loss True (reference data.py:131)")
    if rank == 0:
        print(f'Dataset {args.dataset} loaded.')
    if args.ib:  # train.py:111-113
        dataset_dict['feature_dimensionalities'] = [int(np.sum(dataset_dict['feature_dimensionalities']))]
        dataset_dict['number_features'] = 1
    activation = None if args.activation_fn in ('None', 'none', '') else args.activation_fn
    model = models.DistributedIBNet(
        dataset_dict['feature_dimensionalities'], args.feature_encoder_architecture,
        args.integration_network_architecture,
        dataset_dict['output_dimensionality'] if not args.infonce_loss else args.infonce_shared_dimensionality,  # train.py:116
        use_positional_encoding=args.use_positional_encoding,
        number_positional_encoding_frequencies=args.number_positional_encoding_frequencies, activation_fn=activation,
        feature_embedding_dimension=args.feature_embedding_dimension,
        output_activation_fn=dataset_dict['output_activation_fn'] if not args.infonce_loss else None,
        noise_seed=args.seed, init_seed=args.seed, shuffle_seed=args.seed)
    saver = None
    if args.save_compression_matrices_frequency > 0:
        saver = models.SaveCompressionMatricesCallback(
            args.save_compression_matrices_frequency, dataset_dict['x_valid'],
            dataset_dict.get('x_valid_raw', dataset_dict['x_valid']), args.artifact_outdir,
            one_launch=args.compression_matrices_one_launch)
    # any Keras name; both branches train with it (train.py:128-129, 196, 219), behind the clip / decay arguments that were given
    transforms = dict(clipnorm=args.clipnorm, clipvalue=args.clipvalue, global_clipnorm=args.global_clipnorm,
                      decay=args.learning_rate_decay)
    optimizer = optimizers.get(args.optimizer, **{k: v for k, v in transforms.items() if v is not None})
    optimizer.learning_rate = args.learning_rate
    if args.infonce_loss:  # ---- custom training loop, reference train.py:180-289 ----
        from . import infonce
        F = dataset_dict['number_features']
        if saver is not None:
            saver.set_model(model)
        out = infonce.fit_infonce(
            model, dataset_dict['x_train'], dataset_dict['y_train'], dataset_dict['x_valid'], dataset_dict['y_valid'],
            batch_size=args.batch_size, number_pretraining_epochs=args.number_pretraining_epochs,
            number_annealing_epochs=args.number_annealing_epochs, beta_start=args.beta_start, beta_end=args.beta_end,
            learning_rate=args.learning_rate, y_encoder_architecture=args.infonce_y_encoder_architecture,
            shared_dimensionality=args.infonce_shared_dimensionality, similarity=args.infonce_similarity,
            temperature=args.infonce_temperature, use_positional_encoding=args.use_positional_encoding,
            number_positional_encoding_frequencies=args.number_positional_encoding_frequencies, activation_fn=activation,
            seed=args.seed, optimizer=optimizer,
            # train.py:245-261: the matrices at the epoch boundaries, named by the beta just assigned
            epoch_callback=(lambda epoch, _model: saver.on_epoch_end(epoch)) if saver is not None else None)
        # train.py:271-286: KL and (info based) losses to bits
        kl_series, kl_series_validation = out['kl'] / np.log(2), out['kl_validation'] / np.log(2)
        loss_series, loss_series_validation = out['loss_infonce'], out['loss_infonce_validation']
        if dataset_dict['loss_is_info_based']:
            loss_series, loss_series_validation = loss_series / np.log(2), loss_series_validation / np.log(2)
        if rank == 0:
            print('Finished training.')
            np.savez(os.path.join(args.artifact_outdir, 'history.npz'), beta=np.float32(out['beta']), kl_bits=kl_series,
                     loss=loss_series, kl_bits_validation=kl_series_validation, loss_validation=loss_series_validation)
            visualization.save_distributed_info_plane(kl_series_validation, loss_series_validation, args.artifact_outdir)
            if saver is not None:
                save_compression_matrices_npz(saver, args.artifact_outdir)
        return out
    if args.repeats > 1:
        return train_repeats(args, dataset_dict, optimizer, activation, number_epochs)
    model.compile(optimizer=optimizer, loss=dataset_dict['loss'], metrics=dataset_dict['metrics'])
    callbacks = [models.InfoBottleneckAnnealingCallback(args.beta_start, args.beta_end, args.number_pretraining_epochs,
                                                        args.number_annealing_epochs)]
    if saver is not None:
        callbacks.append(saver)
    history = model.fit(dataset_dict['x_train'], dataset_dict['y_train'], epochs=number_epochs, shuffle=True,
                        batch_size=args.batch_size, callbacks=callbacks, verbose=args.verbose,
                        validation_data=(dataset_dict['x_valid'], dataset_dict['y_valid']),
                        track_information=dict(every=args.info_bounds_frequency) if args.info_bounds_frequency > 0 else None)
    series = postprocess_history(history.history, dataset_dict['number_features'], dataset_dict['loss_is_info_based'])
    beta_series, kl_series, loss_series = series['beta'], series['kl_bits'], series['loss']
    kl_series_validation, loss_series_validation = series['kl_bits_validation'], series['loss_validation']
    if rank == 0:
        print('Finished training.')
        np.savez(os.path.join(args.artifact_outdir, 'history.npz'), beta=beta_series, kl_bits=kl_series,
                 loss=loss_series, kl_bits_validation=kl_series_validation, loss_validation=loss_series_validation)
        visualization.save_distributed_info_plane(kl_series_validation, loss_series_validation, args.artifact_outdir)
        if saver is not None:
            save_compression_matrices_npz(saver, args.artifact_outdir)
        if args.subset_information:
            save_subset_information(dataset_dict, kl_series, loss_series, args.artifact_outdir)
        if history.information is not None:
            info = history.information
            np.savez(os.path.join(args.artifact_outdir, 'info_bounds.npz'), epochs=np.int64(info['epochs']),
                     beta=np.float32(info['beta']), bounds=info['bounds'])
            visualization.save_distributed_info_plane_mi(info, loss_series_validation, args.artifact_outdir)
    return history


if __name__ == '__main__':
    main()
