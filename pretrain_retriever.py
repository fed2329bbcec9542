"""`python pretrain_retriever.py --train_file ... --predict_file ...` -- retriever pre-training, the --do_train loop of the
reference's retrieval/train_retriever.py on one MI355X."""
from proqa_amd.pretrain_retriever import main

if __name__ == "__main__":
    main()
