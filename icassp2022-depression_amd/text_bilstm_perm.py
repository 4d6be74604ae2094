"""Drop-in for Regression/text_bilstm_perm.py on MI355X (SDS-score regressor: 2-layer BiLSTM -> attention ->
Dropout, Linear, ReLU, Dropout, Linear, ReLU; SmoothL1Loss, Adam).  Same `config`, `TextBiLSTM`, `train(epoch) -> train_mae`,
`evaluate(fold, model, train_mae) -> total_loss` and module globals (`train_dep_idxs`, `train_non_idxs`,
`test_dep_idxs`, `test_non_idxs`, `text_features`, `text_targets`, `min_mae`, `min_rmse`)."""
import os

import numpy as np
import torch

from . import _common, models, nn, parallel
from ._common import save  # noqa: F401

prefix = os.path.abspath(os.path.join(os.getcwd(), "../"))
text_features = None
text_targets = None
dep_idxs = None
non_idxs = None

config = {
    'num_classes': 1,
    'dropout': 0.5,
    'rnn_layers': 2,
    'embedding_size': 1024,
    'batch_size': 2,
    'epochs': 110,
    'learning_rate': 1e-5,
    'hidden_dims': 128,
    'bidirectional': True,
    'cuda': False,
    'train_impl': None,      # 9: train() / eval() forwards and the backward on the exchange-free LSTM sweeps (models.TextBiLSTM; H = 128)
}

model = None
optimizer = None
criterion = None
train_dep_idxs = []
train_non_idxs = []
test_dep_idxs = []
test_non_idxs = []
min_mae = 100
min_rmse = 100


def load_features(root=None):
    """Reference lines 17-22: regression features/labels (.npz 'arr_0') and the dep/non index .npy files."""
    global prefix, text_features, text_targets, dep_idxs, non_idxs
    if root is not None:
        prefix = os.path.abspath(root)
    text_features = np.load(os.path.join(prefix, 'Features/TextWhole/whole_samples_reg_avg.npz'))['arr_0']
    text_targets = np.load(os.path.join(prefix, 'Features/TextWhole/whole_labels_reg_avg.npz'))['arr_0']
    dep_idxs = np.load(os.path.join(prefix, 'Features/AudioWhole/dep_idxs.npy'), allow_pickle=True)
    non_idxs = np.load(os.path.join(prefix, 'Features/AudioWhole/non_idxs.npy'), allow_pickle=True)


class TextBiLSTM(models.TextBiLSTM):
    def __init__(self, config, seed=None):
        super().__init__(config, variant='reg', seed=seed)


def train(epoch):
    """Reference lines 131-169."""
    model.train()
    idx = list(train_dep_idxs) + list(train_non_idxs)
    pred_dev = _common.prediction_buffer(len(idx), model.device)       # zero-filled; every rank writes its own rows
    Y_train = text_targets[idx]
    Y_dev = _common.device_labels(Y_train, model.device)
    # config['sample_weights']: None, or 'balanced' = n / (2 * size of its group) per row of the two lists iterated here
    row_weight = _common.sample_row_weight(config, (train_dep_idxs, train_non_idxs))
    W_dev = None if row_weight is None else _common.device_labels(row_weight, model.device)
    feed = _common.FeatureFeeder(text_features, idx, model.device, role='text_features')       # rows of X_train = text_features[idx], in HBM

    def step(a, b, then):
        output = model(feed.rows(a, b, then=then))
        if W_dev is None:
            return criterion(output, Y_dev[a:b].view(-1, 1)), output
        return criterion(output, Y_dev[a:b].view(-1, 1), weight=W_dev[a:b]), output

    def after_step(a, b, output):
        _common.store_predictions(pred_dev, a, output)     # this rank's rows; the others' stay zero until the epoch-end SUM
    total_loss = _common.train_epoch(model, optimizer, len(idx), config['batch_size'], step, after_step, row_weight=row_weight)
    train_mae, train_rmse = _common.epoch_mae_rmse(Y_train, pred_dev)
    if parallel.rank() == 0:
        print('Train Epoch: {:2d}\t Learning rate: {:.4f}\t Loss: {:.4f}\t MAE: {:.4f}\t RMSE: {:.4f}\n '
              .format(epoch + 1, config['learning_rate'], total_loss, train_mae, train_rmse))
    return train_mae


@_common.on_averaged_weights(lambda: optimizer)
def evaluate(fold, model, train_mae):
    """Reference lines 172-210."""
    global min_mae, min_rmse
    model.eval()
    idx = list(test_dep_idxs) + list(test_non_idxs)
    Y_test = text_targets[idx]
    x = _common.FeatureFeeder(text_features, idx, model.device, role='text_features').rows(0, len(idx))
    y = torch.from_numpy(np.ascontiguousarray(Y_test)).type(torch.FloatTensor)
    output = model(x)
    loss = criterion(output, y.view(-1, 1))
    total_loss = loss.item()
    pred = output.data.flatten().cpu().numpy()
    mae, rmse = _common.mae_rmse(Y_test, pred)
    print('MAE: {:.4f}\t RMSE: {:.4f}\n'.format(mae, rmse))
    print('=' * 89)
    if mae <= min_mae and mae < 8.5 and train_mae < 13:
        min_mae, min_rmse = mae, rmse
        save(model, os.path.join(prefix, 'Model/Regression/Text{}/BiLSTM_{}_{:.2f}'.format(
            fold + 1, config['hidden_dims'], min_mae)))
        print('*' * 64)
        print('model saved: mae: {}\t rmse: {}'.format(min_mae, min_rmse))
        print('*' * 64)
    return total_loss


def main(epochs=None):
    """3-fold driver (reference lines 212-256): 10 dep / 44 non test volunteers per fold; the first 14 depressed
    training volunteers are expanded to all 6 time-axis permutations."""
    global model, optimizer, criterion, text_features, text_targets
    global train_dep_idxs, train_non_idxs, test_dep_idxs, test_non_idxs, min_mae, min_rmse
    parallel.init_from_env()
    if text_features is None:
        load_features()
    for fold in range(3):
        test_dep_idxs_tmp = dep_idxs[fold * 10:(fold + 1) * 10]
        test_non_idxs = non_idxs[fold * 44:(fold + 1) * 44]
        train_dep_idxs_tmp = list(set(dep_idxs) - set(test_dep_idxs_tmp))
        train_non_idxs = list(set(non_idxs) - set(test_non_idxs))
        first14 = set(train_dep_idxs_tmp[:14])
        text_features, text_targets, train_dep_idxs = _common.permutation_augment(
            text_features, text_targets, train_dep_idxs_tmp, lambda i: i in first14, (0, 1, 2, 3, 4, 5))
        test_dep_idxs = test_dep_idxs_tmp
        model = TextBiLSTM(config)
        parallel.broadcast_params(model)
        optimizer = nn.Adam(model.parameters(), lr=config['learning_rate'], max_grad_norm=config.get('max_grad_norm'),
                            accumulate_steps=config.get('accum_steps', 1), **_common.optim_options(config))
        criterion = _common.reg_criterion(config, nn.SmoothL1Loss)       # config['loss'] / 'loss_beta' / 'loss_delta'; absent: the reference's
        min_mae = 100; min_rmse = 100
        train_mae = 100
        for ep in range(1, config['epochs'] if epochs is None else epochs):
            train_mae = train(ep)
            evaluate(fold, model, train_mae)


if __name__ == '__main__':
    main()
