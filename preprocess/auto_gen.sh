#!/bin/bash
# Flow and frame selection for one DAVIS-layout sequence (reference: preprocess/auto_gen.sh).
#   bash preprocess/auto_gen.sh camel [vcn_rob.pth]
# Pass 1 keeps the frames that move enough (--flow_threshold 0.05) and installs them as sequence r<seq>; pass 2 computes the
# flow of every consecutive pair (--flow_threshold 0) for <seq> itself.  Without a checkpoint both passes are dry runs.
# Silhouettes must exist under $davisdir/Annotations/$res/<seq>/ first; from one painted frame:
#   python preprocess/propagate_mask.py --datapath $davisdir/JPEGImages/$res/<seq>/ --key 0:first.png --loadmodel vcn_rob.pth
set -e
davisdir=./database/DAVIS
res=Full-Resolution
seqname=$1
newname=r${seqname}
ckpt=${2:-./lasr_vcn/vcn_rob.pth}
load=()
if [ -f "$ckpt" ]; then load=(--loadmodel "$ckpt"); fi
here=$(dirname "$0")

# frames with sufficient motion
python "$here/auto_gen.py" --datapath $davisdir/JPEGImages/$res/$seqname/ "${load[@]}" --testres 1 --outdir ./$newname
for d in JPEGImages Annotations FlowFW FlowBW; do
    mkdir -p $davisdir/$d/$res/$newname
    cp -rf ./$newname/$d/. $davisdir/$d/$res/$newname/
done

# flow of the full sequence
python "$here/auto_gen.py" --datapath $davisdir/JPEGImages/$res/$seqname/ "${load[@]}" --testres 1 --flow_threshold 0 \
    --outdir ./$seqname
for d in FlowFW FlowBW; do
    mkdir -p $davisdir/$d/$res/$seqname
    cp -rf ./$seqname/$d/. $davisdir/$d/$res/$seqname/
done
