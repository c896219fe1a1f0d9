"""Choose the frames to label next from an ``acquisition.npz`` written by ``run_inference --acquisition``:

    python -m bayes_od_rc_amd.select_frames --scores acquisition.npz --by mi_topk --budget N [--class_balanced] [--out list.txt]

writes the chosen frame names, one per line, in rank order (to stdout without ``--out``).
"""
import argparse
import sys

from . import acquisition


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--scores', type=str, required=True, help='acquisition.npz of run_inference --acquisition')
    ap.add_argument('--by', type=str, default='mi_topk', choices=acquisition.COLUMNS, help='the score column frames are ranked by')
    ap.add_argument('--budget', type=int, required=True, help='how many frames to choose (the whole pool when it is smaller)')
    ap.add_argument('--class_balanced', action='store_true', help='greedy selection that evens out the classes the chosen frames '
                    'contain (acquisition.select_frames)')
    ap.add_argument('--out', type=str, default=None, help='file to write the names to (default: stdout)')
    args = ap.parse_args(argv)
    if args.budget < 0:
        ap.error('--budget must be >= 0')
    frames, scores, per_class = acquisition.load(args.scores)
    chosen = acquisition.select_frames(scores, per_class, args.by, args.budget, class_balanced=args.class_balanced)
    names = [frames[i] for i in chosen]
    text = ''.join(n + '\n' for n in names)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text)
    else:
        sys.stdout.write(text)
    return names


if __name__ == '__main__':
    main()
